"""Test-time pipeline for images of different sizes (eval_dan.detect_image_list; csrc/evalpipe_ragged_exact.hip) on the GPU, bit for bit
against what the project computes today: danhip_detect_select against the torch composition it replaces (detect_face's body with
_order_desc, _big_mask / _small_mask, flip_test's mapping), the batched resize against resize_image per item, detect_image_list against
detect_image per image with a deterministic stand-in net and with the real S3FD graph, the absence of host reads, the fixed call counts
(tests/launch_trace.py's recorder around the library calls) and detect_encoded.  No tolerance anywhere: torch.equal.

Launch count of danhip_detect_select: tests/launch_trace.py records library CALLS; the launches inside a call are counted by the call itself
where it issues them (its `launches` output, the idiom of danhip_jpeg_reconstruct_batch) and must equal the documented constant
DANHIP_DETECT_SELECT_LAUNCHES at every A."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evalpipe_standin import FakeNet as _FakeNet, fake_net_np as _fake_net_np, traced as _traced  # noqa: E402

pytestmark = pytest.mark.gpu

SHRINKS = (0.25, 0.75, 1, 1.75, 3.1)
RESIZE_CASES = [(37, 53, 0.5), (64, 48, 0.25), (101, 77, 0.75), (33, 65, 1.25), (40, 40, 1.5), (29, 31, 1.75), (50, 70, 2.0),
                (123, 211, 0.3137), (17, 19, 3.7), (2, 2, 5.0), (480, 640, 0.69)]          # those of test_evalpipe_gpu.test_resize_bit_exact


# ------------------------------------------------------------------------------------------------- 1. select
def _select_inputs(A, kind, dev):
    rng = np.random.RandomState(A * 7 + len(kind))
    cy, cx = rng.rand(A) * 700, rng.rand(A) * 1000
    s = np.exp(rng.rand(A) * np.log(60)) * 4                                 # sides 4 .. 240: both filters cut on both sides at every shrink
    boxes = np.stack([cy - s / 2, cx - s * 0.4, cy + s / 2, cx + s * 0.4], 1).astype(np.float32)
    if kind == "random":
        scores = rng.rand(A).astype(np.float32)
    elif kind == "quantised":
        scores = (np.round(rng.rand(A) * 16) / 16).astype(np.float32)
    else:
        scores = np.full((A,), 0.3125, np.float32)
    return torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev)


def _select_reference(P, bboxes, scores, shrink, filt, mirror_width, max_per_image=750):
    """Today's composition on the same tensors: detect_face's body, the masks of detect_images, flip_test's mapping."""
    s = torch.tensor(float(shrink), dtype=torch.float32, device=bboxes.device)
    det = torch.stack((bboxes[:, 1] / s, bboxes[:, 0] / s, bboxes[:, 3] / s, bboxes[:, 2] / s, scores.to(torch.float32)), dim=1)
    top = min(det.shape[0] - 1, int(max_per_image * 1.5))
    det = det[P._order_desc(det[:, 4])[:top]]
    valid = {0: torch.ones(top, dtype=torch.bool, device=det.device), 1: P._big_mask(det), 2: P._small_mask(det)}[filt]
    if mirror_width is None:
        return det.to(torch.float64), valid
    w = torch.tensor(float(mirror_width), dtype=torch.float32, device=det.device)
    det_t = torch.empty(det.shape, dtype=torch.float64, device=det.device)
    det_t[:, 0] = (w - det[:, 2]) - 1
    det_t[:, 1] = det[:, 1]
    det_t[:, 2] = (w - det[:, 0]) - 1
    det_t[:, 3] = det[:, 3]
    det_t[:, 4] = det[:, 4]
    return det_t, valid


@pytest.mark.parametrize("A", [2, 1126, 1127, 5000, 70001])
def test_select_equals_todays_composition(A, dev):
    from dan_amd import eval_dan as P
    top = min(A - 1, 1125)
    for kind in ("random", "quantised", "equal"):
        bboxes, scores = _select_inputs(A, kind, dev)
        for shrink in SHRINKS:
            for filt in (0, 1, 2):
                for mirror in (None, 1003.0):
                    ref_rows, ref_valid = _select_reference(P, bboxes, scores, shrink, filt, mirror)
                    rows = torch.full((top, 5), -7.0, dtype=torch.float64, device=dev)
                    valid = torch.full((top,), 9, dtype=torch.uint8, device=dev)
                    P.detect_select(bboxes, scores, shrink, top, rows, valid, filt, mirror)
                    what = (A, kind, shrink, filt, mirror)
                    assert torch.equal(rows, ref_rows), what
                    assert torch.equal(valid.bool(), ref_valid) and int(valid.max()) <= 1, what
                    if shrink == 1 and filt and A > 1000:
                        assert 0 < int(ref_valid.sum()) < top, what           # the filter cuts somewhere inside the rows


# ------------------------------------------------------------------------------------------------- 2. batched resize
def test_batched_resize_equals_resize_image_per_item(dev):
    from dan_amd import eval_dan as P
    host = [np.random.RandomState(h * 1000 + w).randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w, _ in RESIZE_CASES]
    offsets, at = [], 1
    for a in host:
        offsets.append(at)
        at += a.size + (3 if a.size % 2 else 2)                                # every start stays odd
    buf = torch.zeros(at + 8, dtype=torch.uint8, device=dev)
    views = []
    for a, off in zip(host, offsets):
        buf[off:off + a.size] = torch.from_numpy(a.reshape(-1)).to(dev)
        views.append(buf[off:off + a.size].view(a.shape))
        assert views[-1].data_ptr() % 2 == 1
    requests = [(i, f, f, m) for m in (0, 1) for i, (_, _, f) in enumerate(RESIZE_CASES)]
    requests += [(10, 1.0, 1.0, 1), (7, 0.5, 1.5, 1)]                          # the plain mirrored copy; fx != fy
    outs = P.resize_image_batch(views, requests)
    assert len(outs) == len(requests)
    for (i, fx, fy, m), got in zip(requests, outs):
        img = torch.from_numpy(host[i]).to(dev)
        ref = P.resize_image(img.flip(1).contiguous() if m else img, fx, fy)
        assert got.shape == ref.shape and torch.equal(got, ref), (i, fx, fy, m)
    assert torch.equal(outs[-2], torch.from_numpy(host[10]).to(dev).flip(1))


# ------------------------------------------------------------------------------------------------- 3. the list pipeline, stand-in net
class _CachedNet(object):
    """A stand-in that reads nothing back: its answer depends on the image SIZE only and is built once per size (the warm-up call)."""

    def __init__(self):
        self.cache = {}

    def __call__(self, image):
        key = (int(image.shape[0]), int(image.shape[1]))
        if key not in self.cache:
            b, s = _fake_net_np(np.zeros(key + (3,), np.uint8))
            self.cache[key] = (torch.from_numpy(b).to(image.device), torch.from_numpy(s).to(image.device))
        return self.cache[key]


def _images(sizes, seed, dev):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).to(dev) for h, w in sizes]


def _same_as_serial(P, net, imgs, pyramid):
    out, num = P.detect_image_list(net, imgs, pyramid=pyramid)
    assert out.shape == (len(imgs), P.MAX_PER_IMAGE, 5) and out.dtype == torch.float32 and num.dtype == torch.int32
    for b, im in enumerate(imgs):
        ref = P.detect_image(net, im, pyramid=pyramid)
        n = int(num[b].item())
        assert n == ref.shape[0] and n > 5, (b, n, ref.shape)
        assert torch.equal(out[b, :n], ref), b


@pytest.mark.parametrize("pyramid", [True, False])
def test_list_pipeline_equals_detect_image_per_image(pyramid, dev):
    from dan_amd import eval_dan as P
    sizes = [(240, 320), (203, 331), (400, 300), (120, 160)]
    assert P.get_shrink(120, 160)[1] > 2                                       # the loop branch of multi_scale_test
    _same_as_serial(P, _FakeNet(), _images(sizes, 31, dev), pyramid)


def test_eval_sfd_reexport_has_no_pyramid_pass(dev):
    from dan_amd import eval_dan as P, eval_sfd as PS
    imgs = _images([(203, 331), (120, 160)], 32, dev)
    a, na = PS.detect_image_list(_FakeNet(), imgs)
    b, nb = P.detect_image_list(_FakeNet(), imgs, pyramid=False)
    assert torch.equal(na, nb) and torch.equal(a[0, :int(na[0])], b[0, :int(nb[0])])


# ------------------------------------------------------------------------------------------------- 4. the real S3FD graph
def test_list_pipeline_real_network(dev):
    """Each forward is the same batch-1 shape on both sides, so equality is bitwise (as test_batched_pipeline_real_network argues)."""
    from dan_amd import eval_dan as P
    from dan_amd import train_sfd
    imgs = _images([(203, 331), (160, 250)], 9, dev)
    net = P.Detector(train_sfd.SFDModel(device=dev), lambda h, w, d: train_sfd.AnchorConfig(h, w, d))
    out, num = P.detect_image_list(net, imgs, pyramid=False)
    for b, im in enumerate(imgs):
        ref = P.detect_image(net, im, pyramid=False)
        n = int(num[b].item())
        assert n == ref.shape[0] and torch.equal(out[b, :n], ref), b


# ------------------------------------------------------------------------------------------------- 5. no host read, fixed call counts
def test_no_host_read_between_the_first_launch_and_the_return(dev):
    from dan_amd import eval_dan as P
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("this torch build has no sync debug mode")
    net, imgs = _CachedNet(), _images([(240, 320), (203, 331), (120, 160)], 33, dev)
    warm = P.detect_image_list(net, imgs)                                      # fills the stand-in's cache
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out, num = P.detect_image_list(net, imgs)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(num, warm[1]) and int(num.min()) > 5


def test_one_resize_call_and_one_vote_call_whatever_the_list(dev):
    from dan_amd import eval_dan as P
    net = _CachedNet()
    for sizes, pyramid in (([(203, 331)], False), ([(240, 320), (203, 331), (400, 300)], True), ([(120, 160), (64, 48), (300, 500), (90, 700), (33, 65)], True)):
        imgs = _images(sizes, 34, dev)
        _, names = _traced(P, lambda: P.detect_image_list(net, imgs, pyramid=pyramid))
        passes = sum(len(P.scale_passes(h, w, pyramid)) for h, w in sizes)
        assert names.count("danhip_resize_u8_linear_batch") == 1 and names.count("danhip_bbox_vote") == 1, names
        assert names.count("danhip_detect_select") == passes
        assert names.count("danhip_argsort_desc_f32") == len(sizes)           # the vote's per-image order; none per pass
        assert "danhip_resize_u8_linear" not in names


@pytest.mark.parametrize("A", [5000, 70001])
def test_select_launch_count_is_the_documented_constant(A, dev):
    from dan_amd import _lib, eval_dan as P
    bboxes, scores = _select_inputs(A, "random", dev)
    rows = torch.empty((1125, 5), dtype=torch.float64, device=dev)
    valid = torch.empty((1125,), dtype=torch.uint8, device=dev)
    launches, names = _traced(P, lambda: P.detect_select(bboxes, scores, 1.0, 1125, rows, valid))
    assert names == ["danhip_detect_select"]
    assert launches == _lib.DETECT_SELECT_LAUNCHES == 7


# ------------------------------------------------------------------------------------------------- 6. detect_encoded
def test_detect_encoded_equals_the_list_pipeline_on_pillow_decodes(dev):
    Image = pytest.importorskip("PIL.Image")
    from dan_amd import eval_dan as P
    from dan_amd.dataset.jpeg import JpegDecoder
    datas, arrays = [], []
    for k, (h, w) in enumerate([(120, 160), (97, 131), (150, 111)]):
        rng = np.random.RandomState(50 + k)
        img = (rng.rand(h // 8 + 1, w // 8 + 1, 3) * 255).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        b = io.BytesIO()
        Image.fromarray(img).save(b, format="JPEG", quality=92, progressive=(k == 1))
        datas.append(b.getvalue())
        arrays.append(np.asarray(Image.open(io.BytesIO(datas[-1])).convert("RGB")).copy())
    dec = JpegDecoder(dev)
    out, num = P.detect_encoded(_FakeNet(), datas, dec)
    assert dec.stats["device"] == 2 and dec.stats["fallback"] == {"progressive": 1}
    ref, ref_num = P.detect_image_list(_FakeNet(), [torch.from_numpy(a).to(dev) for a in arrays])
    assert torch.equal(num, ref_num) and int(num.min()) > 5
    for b in range(3):
        assert torch.equal(out[b, :int(num[b])], ref[b, :int(num[b])]), b
