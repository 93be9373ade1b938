"""The three forms of the test-time pipeline (eval_dan.detect_image / detect_images / detect_image_list) walk one scale plan: bit for bit the
same detections on every branch of the schedule, at every setting of the parameters they share, with the call counts the plan implies.

multi_scale_test's schedule has four branches in max_shrink (> 2: the doubling loop; 1 < m <= 2; 0.75 <= m <= 1; m < 0.75).  At the default
memory_limit the last two need images of about 1100 x 1500 and more; memory_limit moves a 120 x 160 and a 96 x 136 image through all four
(max_shrink per limit: tests/test_evalpipe_ragged_cpu.py pins the table).  At 80000 and 115000 the two sizes sit on different branches, so
the list form walks two branches in one call; at 80000 the 120 x 160 image has shrink != 1, so its mirrored pass is a resized one too.
The network is the deterministic stand-in (tests/evalpipe_standin.py): every case is a few launches on tiny images.  No tolerance: torch.equal."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from evalpipe_standin import ANCHORS, FakeNet, traced  # noqa: E402

pytestmark = pytest.mark.gpu

LIMITS = (577, 40000, 80000, 115000, 150000)
SIZES = ((120, 160), (96, 136), (120, 160))
_SERIAL = {}                     # (image, pyramid, memory_limit, max_per_image) -> detect_image's answer, computed once


def _images(dev):
    return [torch.from_numpy(np.random.RandomState(40 + k).randint(0, 256, (h, w, 3)).astype(np.uint8)).to(dev) for k, (h, w) in enumerate(SIZES)]


def _serial(P, imgs, k, pyramid, memory_limit, max_per_image=750):
    key = (k, pyramid, memory_limit, max_per_image)
    if key not in _SERIAL:
        _SERIAL[key] = P.detect_image(FakeNet(), imgs[k], pyramid, max_per_image=max_per_image, memory_limit=memory_limit)
    return _SERIAL[key]


def _equal(P, imgs, which, out, num, pyramid, memory_limit, max_per_image=750):
    """Rows [0, num[b]) of image b against detect_image on imgs[which[b]] -> the counts."""
    assert out.shape == (len(which), max_per_image, 5) and out.dtype == torch.float32 and num.dtype == torch.int32
    counts = num.tolist()
    for b, k in enumerate(which):
        ref = _serial(P, imgs, k, pyramid, memory_limit, max_per_image)
        assert counts[b] == ref.shape[0], (b, counts[b], ref.shape)
        assert torch.equal(out[b, :counts[b]], ref), b
    return counts


@pytest.mark.parametrize("pyramid", [True, False])
@pytest.mark.parametrize("memory_limit", LIMITS)
def test_same_size_batch_equals_detect_image(memory_limit, pyramid, dev):
    from dan_amd import eval_dan as P
    imgs = _images(dev)
    out, num = P.detect_images(FakeNet(), torch.stack((imgs[0], imgs[2])), pyramid, memory_limit=memory_limit)
    assert min(_equal(P, imgs, (0, 2), out, num, pyramid, memory_limit)) > 5


@pytest.mark.parametrize("pyramid", [True, False])
@pytest.mark.parametrize("memory_limit", LIMITS)
def test_mixed_size_list_equals_detect_image(memory_limit, pyramid, dev):
    from dan_amd import eval_dan as P
    imgs = _images(dev)
    out, num = P.detect_image_list(FakeNet(), imgs, pyramid, memory_limit=memory_limit)
    assert min(_equal(P, imgs, (0, 1, 2), out, num, pyramid, memory_limit)) > 5


def test_the_cut_and_the_cap_follow_max_per_image_in_all_three_forms(dev):
    """max_per_image = 8: every pass keeps int(1.5 * 8) = 12 of the stand-in's 1500 rows (1125 at the default), and the vote returns at most 8.
    Both bind: the 12-row passes of the loop branch vote into 12 or 13 clusters (oracle/evalpipe.py on the same stand-in and images), so
    the cap cuts too and every count is exactly 8."""
    from dan_amd import eval_dan as P
    mpi = 8
    cut = int(mpi * 1.5)
    imgs = _images(dev)
    assert cut < ANCHORS - 1 and FakeNet()(imgs[0])[1].shape[0] == ANCHORS
    assert P.detect_face(FakeNet(), imgs[0], 1, mpi).shape[0] == cut                     # the cut binds
    assert P.detect_face(FakeNet(), imgs[0], 1).shape[0] == int(P.MAX_PER_IMAGE * 1.5) > cut    # below the default's cut
    out, num = P.detect_images(FakeNet(), torch.stack((imgs[0], imgs[2])), True, max_per_image=mpi)
    assert _equal(P, imgs, (0, 2), out, num, True, 577.0, mpi) == [mpi, mpi]
    out, num = P.detect_image_list(FakeNet(), imgs, True, max_per_image=mpi)
    assert _equal(P, imgs, (0, 1, 2), out, num, True, 577.0, mpi) == [mpi, mpi, mpi]


@pytest.mark.parametrize("memory_limit", [577, 115000])
def test_call_counts_are_those_of_the_plan(memory_limit, dev):
    """detect_image shows the network one image per pass; detect_images runs one batched forward per pass and ONE voting call.  Around
    them: one resize per image and pass whose scale is not 1, one arg-sort per image and pass for the cut, one per image for the vote."""
    from dan_amd import eval_dan as P
    imgs = _images(dev)
    batch = torch.stack((imgs[0], imgs[2]))
    passes = P.scale_passes(120, 160, True, memory_limit)
    resized = sum(1 for scale, _, _ in passes if scale != 1)
    assert len(passes) == {577: 12, 115000: 5}[memory_limit] and resized == {577: 10, 115000: 5}[memory_limit]
    net = FakeNet()
    _, names = traced(P, lambda: P.detect_image(net, imgs[0], True, memory_limit=memory_limit))
    assert (net.shown, net.batches) == (len(passes), 0)
    assert names.count("danhip_bbox_vote") == 1 and names.count("danhip_resize_u8_linear") == resized
    assert names.count("danhip_argsort_desc_f32") == len(passes) + 1
    net = FakeNet()
    _, names = traced(P, lambda: P.detect_images(net, batch, True, memory_limit=memory_limit))
    assert (net.shown, net.batches) == (0, len(passes))
    assert names.count("danhip_bbox_vote") == 1 and names.count("danhip_resize_u8_linear") == 2 * resized
    assert names.count("danhip_argsort_desc_f32") == 2 * len(passes) + 2
    assert set(names) == {"danhip_bbox_vote", "danhip_resize_u8_linear", "danhip_argsort_desc_f32"}
