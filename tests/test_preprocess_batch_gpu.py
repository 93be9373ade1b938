"""The batched device pass of the training input pipeline (danhip_augment_preprocess_batch through dan_preprocessing.augment_batch) and the
three preprocessing surfaces on it: every slice against the oracle chain (oracle/preprocess.py) and against the per-image entry point,
isolation between the items of a batch, the edges of the grid, sources that are views at odd byte offsets, the batched pipelines against
successive per-image calls, the record reader, and one network forward.

Slices are compared by equality (tests/augment_exact.py: assert_exact - the oracle's float32 result rounded to the 16-bit type, no value may
differ).  An item WITHOUT a contrast op sums nothing across workgroups, so its slice equals augment_image's bit for bit; so does an item WITH
one when its mean cannot depend on the summation order - tests/test_augment_exact_cpu.py establishes that for the items that
pinned_contrast_items() lists (the tables of this file).  The chains of the drawn pipelines are not in that list: for them the comparison
with the per-image result keeps its bound (fewer than 2e-3 of the values differ, none by more than 1.01).
Launch count: the project's launch trace (tests/launch_trace.py) records the calls of dan_amd/ops.py, not launches inside the library, so the
constant (1 launch, 3 with a contrast op, for any B) is documented in include/danhip.h and read from a kernel trace in profiles/r13/augment_batch.md."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_exact as AE  # noqa: E402

pytestmark = pytest.mark.gpu
ANCHOR_SCALES = [16., 32., 64., 128., 256., 512.]
SIZES = [(50, 60), (96, 128), (333, 333), (200, 900), (413, 577)]
OUT_SHAPES = [(80, 80), (64, 96)]
ALL4 = {"first": [("contrast", 1.3), ("hue", 0.1), ("brightness", -0.05), ("saturation", 1.2)],
        "middle": [("saturation", 0.7), ("brightness", 0.08), ("contrast", 0.6), ("hue", -0.15)],
        "last": [("brightness", 0.1), ("saturation", 1.4), ("hue", 0.17), ("contrast", 1.5)]}
# two batches of B = 5 over the five sizes: (ops, window (y, x, h, w), flip)
BATCHES = {
    "single_ops": [([], (5, 7, 40, 45), False),                                           # no ops, window inside the image
                   ([("brightness", 0.1)], (-20, -10, 150, 160), True),                     # leaves the 96 x 128 image on every side
                   ([("saturation", 1.4)], (100, 50, 200, 120), True),
                   ([("hue", -0.2)], (0, 0, 200, 900), False),
                   ([("contrast", 0.5)], (13, 29, 377, 401), False)],
    "all_four": [(ALL4["first"], (-8, -9, 70, 80), False),                                  # leaves the 50 x 60 image on every side
                 (ALL4["middle"], (10, 20, 60, 90), True),
                 (ALL4["last"], (33, 1, 300, 299), False),
                 ([], (1500, 1500, 16, 16), False),                                         # entirely outside the image
                 ([("hue", 0.1), ("saturation", 1.2), ("contrast", 1.1), ("brightness", -0.1)], (-30, 400, 300, 300), True)],
}


def _image(seed, h, w):
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.float32)
    img = np.kron(base, np.ones((8, 8, 1), np.float32))[:h, :w] + rng.randn(h, w, 3) * 12          # blocky + noise, as tests/test_preprocess_gpu.py
    return np.clip(img, 0, 255).astype(np.uint8)


def _boxes(seed, h, w, n):
    rng = np.random.RandomState(seed)
    cy, cx = rng.rand(n) * h, rng.rand(n) * w
    s = np.exp(rng.rand(n) * np.log(12)) * 10
    return np.stack([np.clip(cy - s / 2, 0, h - 1), np.clip(cx - s / 2, 0, w - 1), np.clip(cy + s / 2, 0, h - 1), np.clip(cx + s / 2, 0, w - 1)],
                    1).astype(np.float32)


def _has_contrast(ops):
    return any(n == "contrast" for n, _ in ops)


def _oracle(img, ops, win, flip, out_shape, flip_window=False):
    return AE.oracle(img, ops, win, AE.FLIP_WINDOW if flip_window else int(bool(flip)), out_shape)


_close = AE.assert_exact          # (got [h, w, 8] slice of the device result, float32 [h, w, 3] reference before the 16-bit rounding, what)


def _bounded(got, ref32, what):
    """The bound of the per-image comparison for a contrast item whose mean's order-independence nothing establishes."""
    g = got.float().cpu().numpy()
    assert np.all(g[..., 3:] == 0), what
    ref16 = torch.from_numpy(np.ascontiguousarray(ref32)).to(got.dtype).float().numpy()
    d = np.abs(g[..., :3] - ref16)
    assert (d > 0).mean() < 2e-3 and d.max() <= 1.01, (what, (d > 0).mean(), d.max())


def _same_as_per_image(got, per_image, ops, what, pinned=True):
    """pinned: the item is one of pinned_contrast_items() (or has no contrast op): bit for bit."""
    if _has_contrast(ops) and not pinned:                                         # the mean's fp64 sum crosses workgroups in another order
        _bounded(got, per_image.float().cpu().numpy()[..., :3], what)
        assert torch.all(got[..., 3:] == 0)
    else:
        assert torch.equal(got, per_image), what


def _grid_case():
    """Host images and items of test_grid_edges_one_image_and_seventeen: (big, its item, the 17 images, the 17 items)."""
    big = _image(40, 700, 500)
    tiny = [_image(50 + i, 8, 8) for i in range(16)]
    imgs = tiny[:8] + [big] + tiny[8:]
    items = [([("contrast", 1.2)] if i % 3 == 0 else [("hue", 0.05 * (i % 5))], (i % 3 - 1, 1 - i % 2, 6 + i % 4, 8), bool(i % 2)) for i in range(17)]
    items[8] = (ALL4["middle"], (-10, 5, 650, 480), False)
    return big, (ALL4["last"], (50, 60, 500, 400), True), imgs, items


def pinned_contrast_items():
    """(name, host image, ops) of every contrast item that this file compares bit for bit with the per-image entry point; the condition
    itself is asserted without a GPU by tests/test_augment_exact_cpu.py."""
    for name, items in sorted(BATCHES.items()):
        for k, (ops, _, _) in enumerate(items):
            if _has_contrast(ops):
                yield "%s item %d" % (name, k), _image(20 + k, *SIZES[k]), ops
    big, item, imgs, items = _grid_case()
    yield "grid B = 1", big, item[0]
    for k, (ops, _, _) in enumerate(items):
        if _has_contrast(ops):
            yield "grid B = 17 item %d" % k, imgs[k], ops


@pytest.fixture(scope="module")
def images(dev):
    host = [_image(20 + i, h, w) for i, (h, w) in enumerate(SIZES)]
    return host, [torch.from_numpy(a).to(dev) for a in host]


@pytest.fixture(scope="module")
def batch_results(images):
    """The four batched calls (two item sets x two output shapes), run once and shared."""
    from dan_amd.preprocessing import dan_preprocessing as P
    return {(name, out_shape): P.augment_batch(images[1], items, out_shape) for name, items in BATCHES.items() for out_shape in OUT_SHAPES}


@pytest.mark.parametrize("out_shape", OUT_SHAPES)
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_batch_against_the_oracle(name, out_shape, images, batch_results):
    out = batch_results[(name, out_shape)]
    assert tuple(out.shape) == (5, out_shape[0], out_shape[1], 8)
    for k, (ops, win, flip) in enumerate(BATCHES[name]):
        _close(out[k], _oracle(images[0][k], ops, win, flip, out_shape), "%s item %d %s" % (name, k, out_shape))
    if name == "all_four":                                                        # item 3: exactly the mean colour -> trunc(mean * 255.5 / 255) - mean
        means = np.asarray([103.94, 116.78, 123.68], np.float32)
        exp = np.trunc(means / np.float32(255.) * np.float32(255.5)) - means
        exp16 = torch.tensor(exp).to(out.dtype).float().numpy()
        far = out[3].float().cpu().numpy()
        assert np.array_equal(far[..., :3], np.broadcast_to(exp16, far[..., :3].shape))


@pytest.mark.parametrize("out_shape", OUT_SHAPES)
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_batch_against_the_per_image_entry_point(name, out_shape, images, batch_results):
    from dan_amd.preprocessing import dan_preprocessing as P
    out = batch_results[(name, out_shape)]
    for k, (ops, win, flip) in enumerate(BATCHES[name]):
        _same_as_per_image(out[k], P.augment_image(images[1][k], ops, win, flip, out_shape), ops, "%s item %d" % (name, k))


def test_flip_of_the_window_before_the_resize(images):
    """FLIP_WINDOW (sfd_preprocessing.py:522 before :531): the oracle's crop mirrored, then resized - not the resized image mirrored."""
    from dan_amd.preprocessing import dan_preprocessing as P
    items = [([], (5, 7, 40, 45), P.FLIP_WINDOW), (ALL4["middle"], (-20, -10, 150, 160), P.FLIP_WINDOW), ([("hue", 0.1)], (100, 50, 200, 120), P.FLIP_RESIZED)]
    out = P.augment_batch(images[1][:3], items, (64, 96))
    for k, (ops, win, flip) in enumerate(items):
        _close(out[k], _oracle(images[0][k], ops, win, True, (64, 96), flip_window=flip == P.FLIP_WINDOW), "flip mode %d item %d" % (flip, k))
    other = _oracle(images[0][0], [], (5, 7, 40, 45), True, (64, 96))             # the two orders are different images
    assert np.abs(other - _oracle(images[0][0], [], (5, 7, 40, 45), True, (64, 96), flip_window=True)).max() > 1


def test_items_of_a_batch_do_not_leak_into_each_other(images, dev):
    """Second run with item 2's image, ops and window changed: every other slice stays bit-identical (a segment boundary of the mean
    reduction or a tile-to-image mapping that leaks would show).  An item's fp64 mean sum is a few hundred workgroup partials at most; its
    arrival order can move the float mean only when the sum sits within 1e-16 of a rounding boundary."""
    from dan_amd.preprocessing import dan_preprocessing as P
    items = list(BATCHES["all_four"])
    first = P.augment_batch(images[1], items, (80, 80)).clone()
    other = torch.from_numpy(_image(99, 150, 170)).to(dev)
    items2 = list(items)
    items2[2] = ([("contrast", 0.5), ("brightness", 0.1)], (-3, 20, 100, 160), True)
    second = P.augment_batch(images[1][:2] + [other] + images[1][3:], items2, (80, 80))
    for k in (0, 1, 3, 4):
        assert torch.equal(first[k], second[k]), k
    assert not torch.equal(first[2], second[2])
    _close(second[2], _oracle(_image(99, 150, 170), items2[2][0], items2[2][1], True, (80, 80)), "changed item")


@pytest.mark.parametrize("out_shape", [(8, 8), (160, 160)])
def test_grid_edges_one_image_and_seventeen(out_shape, dev):
    from dan_amd.preprocessing import dan_preprocessing as P
    big_host, (ops1, win1, flip1), hosts, items = _grid_case()
    big = torch.from_numpy(big_host).to(dev)
    one = P.augment_batch([big], [(ops1, win1, flip1)], out_shape)
    _same_as_per_image(one[0], P.augment_image(big, ops1, win1, flip1, out_shape), ops1, "B = 1")
    imgs = [big if a is big_host else torch.from_numpy(a).to(dev) for a in hosts]
    out = P.augment_batch(imgs, items, out_shape)
    assert tuple(out.shape) == (17,) + tuple(out_shape) + (8,)
    for k, (ops, win, flip) in enumerate(items):
        _same_as_per_image(out[k], P.augment_image(imgs[k], ops, win, flip, out_shape), ops, "B = 17 item %d" % k)


def test_sources_as_views_at_odd_byte_offsets(images, batch_results, dev):
    from dan_amd.preprocessing import dan_preprocessing as P
    offsets, at = [], 1
    for a in images[0]:
        offsets.append(at)
        at += a.size + (3 if a.size % 2 else 2)                                   # every start stays odd: 1, 3 mod 4 both occur
    buf = torch.zeros(at + 8, dtype=torch.uint8, device=dev)
    views = []
    for a, off in zip(images[0], offsets):
        buf[off:off + a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
        views.append(buf[off:off + a.size].view(a.shape))
        assert views[-1].data_ptr() % 2 == 1
    assert {v.data_ptr() % 4 for v in views} == {1, 3}
    for name, items in BATCHES.items():
        out = P.augment_batch(views, items, (64, 96))
        for k, (ops, _, _) in enumerate(items):
            _same_as_per_image(out[k], batch_results[(name, (64, 96))][k], ops, "%s view %d" % (name, k))


def _pipeline_inputs(dev):
    host = [_image(60 + i, h, w) for i, (h, w) in enumerate([(96, 128), (413, 577), (240, 320), (200, 300)])]
    boxes = [_boxes(70 + i, a.shape[0], a.shape[1], n) for i, (a, n) in enumerate(zip(host, (3, 1, 6, 4)))]
    boxes[1] = np.asarray([[200., 300., 203., 303.]], np.float32)                  # a 3 x 3 face of the 413 x 577 image: gone at 64 x 64
    return [torch.from_numpy(a).to(dev) for a in host], boxes


@pytest.mark.parametrize("module", ["dan_preprocessing", "pb_preprocessing", "sfd_preprocessing"])
@pytest.mark.parametrize("seed", [3, 4])
def test_batched_pipeline_equals_successive_per_image_calls(module, seed, dev):
    import importlib
    M = importlib.import_module("dan_amd.preprocessing." + module)
    imgs, boxes = _pipeline_inputs(dev)
    extra = () if module == "sfd_preprocessing" else (ANCHOR_SCALES,)
    d = M.Draws(seed)
    singles = [M.preprocess_for_train(im, b, (64, 64), *extra, draws=d) for im, b in zip(imgs, boxes)]
    out, out_boxes, kept = M.preprocess_batch_for_train(imgs, boxes, (64, 64), *extra, draws=M.Draws(seed))
    assert kept == [k for k, (_, b) in enumerate(singles) if len(b)] and 1 not in kept and len(kept) == 3
    assert tuple(out.shape) == (3, 64, 64, 8) and len(out_boxes) == 3
    for j, k in enumerate(kept):
        assert np.array_equal(out_boxes[j], singles[k][1]), (module, k)           # same draws -> same window, flip and boxes
        _same_as_per_image(out[j], singles[k][0], [("contrast", 1.0)], "%s image %d" % (module, k), pinned=False)    # (the chain always has a contrast op)


def test_sfd_window_and_flip_of_the_batch_are_those_of_the_draws(dev):
    """The image of sfd_preprocessing.preprocess_batch_for_train is the oracle chain for the window, ops and flip that draw_for_train draws."""
    from dan_amd.preprocessing import sfd_preprocessing as S
    imgs, boxes = _pipeline_inputs(dev)
    out, out_boxes, kept = S.preprocess_batch_for_train(imgs, boxes, (64, 64), draws=S.Draws(9))
    d, j = S.Draws(9), 0
    for k, (im, b) in enumerate(zip(imgs, boxes)):
        ops, win, flip, bx = S.draw_for_train(im.shape[0], im.shape[1], b, (64, 64), d)
        if not len(bx):
            continue
        assert kept[j] == k and np.array_equal(out_boxes[j], bx)
        _close(out[j], _oracle(im.cpu().numpy(), ops, win, flip, (64, 64), flip_window=flip), "sfd image %d" % k)
        j += 1
    assert j == len(kept)


def test_record_reader_with_the_batched_pass_equals_the_per_image_path(dev, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from dan_amd.dataset import dataset_common as DC
    from dan_amd.preprocessing import sfd_preprocessing as S
    recs = []
    for i in range(10):                                                           # the records of tests/test_jpeg_gpu.py
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

    def pixels(image, bboxes):
        h, w = image.shape[:2]
        return np.asarray(bboxes, np.float32).reshape(-1, 4) * np.asarray([h, w, h, w], np.float32)

    def encoder(b):
        return [b * np.float32(0.5)], [np.ones((len(b),), np.int64)], [np.zeros((len(b),), np.float32)], [b]

    def run(batched):
        draws, calls = S.Draws(11), []

        def prep(image, bboxes):
            if len(bboxes) == 0:
                return None, []
            return S.preprocess_for_train(image, pixels(image, bboxes), (128, 128), draws=draws)

        def prep_batch(images, bboxes_list):
            calls.append(len(images))
            return S.preprocess_batch_for_train(images, [pixels(im, b) for im, b in zip(images, bboxes_list)], (128, 128), draws=draws)

        entries = []
        for batch in DC.slim_get_batch(2, 3, "train", pattern, 2, 2, prep, encoder, num_epochs=2, is_training=True, seed=1, decode_device=dev,
                                       batch_preprocessing_fn=prep_batch if batched else None):
            assert len(batch) == 3
            entries += batch
        return entries, calls

    per_image, no_calls = run(False)
    batched, calls = run(True)
    assert no_calls == [] and len(calls) >= 6 and max(calls) == 3                   # every decoded group went through the batched pass once
    assert len(per_image) == len(batched) >= 6
    for a, b in zip(per_image, batched):
        assert a[1] == b[1] and np.array_equal(a[2], b[2]) and len(a) == len(b) == 7
        for x, y in zip(a[3:], b[3:]):                                            # anchor targets, labels, scores, boxes
            assert np.array_equal(x, y)
        assert tuple(b[0].shape) == (128, 128, 8)
        _same_as_per_image(b[0], a[0], [("contrast", 1.0)], a[1], pinned=False)


def test_batch_feeds_the_network(dev):
    from dan_amd.preprocessing import sfd_preprocessing as S
    from dan_amd.train_sfd import SFDModel
    imgs = [torch.from_numpy(_image(80 + i, h, w)).to(dev) for i, (h, w) in enumerate([(300, 420), (240, 320)])]
    boxes = [_boxes(90 + i, int(im.shape[0]), int(im.shape[1]), 8) for i, im in enumerate(imgs)]
    x, b, kept = S.preprocess_batch_for_train(imgs, boxes, (128, 128), draws=S.Draws(5))
    assert tuple(x.shape) == (2, 128, 128, 8) and kept == [0, 1]
    model = SFDModel(device=dev)
    with torch.no_grad():
        feats = model.backbone.get_featmaps(x, training=False)
    assert feats[0].shape[1:3] == (32, 32) and all(torch.isfinite(f.float()).all() for f in feats)
