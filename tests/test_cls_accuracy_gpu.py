"""danhip_cls_accuracy (csrc/loss.hip) against a numpy restatement of the reference's metric - tf.metrics.accuracy(clip(labels, 0, num_classes)
[final_mask], argmax(cls_pred[final_mask], -1)), train_sfd.py:383-390 - with exact integer equality in every case."""
import functools
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "include", "danhip.h")).read()
THREADS = int(re.search(r"#define DANHIP_CLS_ACCURACY_THREADS (\d+)", _HDR).group(1))
MAX_BLOCKS = int(re.search(r"#define DANHIP_CLS_ACCURACY_MAX_BLOCKS (\d+)", _HDR).group(1))
LOOPS = THREADS * MAX_BLOCKS + 1              # one anchor more than a full grid covers in one round: workgroup 0 takes a second round
PARTLY_EMPTY = 3 * THREADS + 5                # four workgroups, the last with 5 of its lanes in range (B = 1)
SIZES = (1, 63, 64, 65, 257, PARTLY_EMPTY, LOOPS)


def reference(cls, labels, sel):
    """{correct, total} of the reference's cls_accuracy for one step."""
    mask = sel.reshape(-1) != 0                                          # final_mask
    pred = np.argmax(cls.reshape(-1, 2), axis=-1)[mask]                  # first index on equal logits, as tf.argmax
    target = np.clip(labels.reshape(-1), 0, 2)[mask]                     # tf.clip_by_value(cls_targets, 0, num_classes)
    return np.array([np.count_nonzero(pred == target), np.count_nonzero(mask)], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def case(B, A):
    """Labels from {-1, 0, 1} and sel from {0, 1, 2}, independently; logits from a small set of values so that equal pairs occur anywhere.
    With B = 3: row 1 has EVERY pair of logits equal (ties go to class 0), row 2 has sel all zero (it adds nothing)."""
    rng = np.random.RandomState(1000 * B + A % 997)
    cls = rng.randint(-3, 4, size=(B, A, 2)).astype(np.float32) * np.float32(0.5)
    labels = rng.randint(-1, 2, size=(B, A)).astype(np.int32)
    sel = rng.randint(0, 3, size=(B, A)).astype(np.uint8)
    if B == 3:
        cls[1, :, 1] = cls[1, :, 0]
        sel[2] = 0
    for a in (cls, labels, sel):
        a.setflags(write=False)
    return cls, labels, sel, reference(cls, labels, sel)


def _run(dev, cls, labels, sel, counts=None):
    from dan_amd import ops
    counts = torch.zeros(2, dtype=torch.int64, device=dev) if counts is None else counts
    ops.cls_accuracy(torch.tensor(cls, device=dev), torch.tensor(labels, device=dev), torch.tensor(sel, device=dev), counts)
    return counts


@pytest.mark.parametrize("A", SIZES)
@pytest.mark.parametrize("B", (1, 3))
def test_counts_equal_the_numpy_restatement(dev, B, A):
    cls, labels, sel, want = case(B, A)
    got = _run(dev, cls, labels, sel).cpu().numpy()
    assert 0 <= want[0] <= want[1] <= B * A
    assert np.array_equal(got, want), (B, A, got, want)


def test_equal_logits_count_as_class_zero(dev):
    A = 257
    cls = np.repeat(np.linspace(-2, 2, A, dtype=np.float32)[None, :, None], 2, axis=2)      # every pair equal
    sel = np.ones((1, A), np.uint8)
    for label, correct in ((0, A), (1, 0), (-1, A)):                                       # -1 clips to 0
        labels = np.full((1, A), label, np.int32)
        assert np.array_equal(reference(cls, labels, sel), [correct, A])
        assert _run(dev, cls, labels, sel).tolist() == [correct, A]
    cls2 = cls.copy()
    cls2[0, :, 1] = np.nextafter(cls2[0, :, 1], np.float32(np.inf))                        # one ulp above: class 1
    assert _run(dev, cls2, np.full((1, A), 1, np.int32), sel).tolist() == [A, A]


def test_nothing_selected_adds_nothing(dev):
    cls, labels, _, _ = case(3, 257)
    counts = torch.tensor([7, 11], dtype=torch.int64, device=dev)
    _run(dev, cls, labels, np.zeros((3, 257), np.uint8), counts)
    assert counts.tolist() == [7, 11]


def test_two_calls_accumulate(dev):
    a, b = case(3, 65), case(1, LOOPS)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    _run(dev, *a[:3], counts=counts)
    _run(dev, *b[:3], counts=counts)
    _run(dev, *a[:3], counts=counts)
    assert np.array_equal(counts.cpu().numpy(), 2 * a[3] + b[3])
    big = torch.tensor([1 << 40, (1 << 40) + 5], dtype=torch.int64, device=dev)            # the counters are 64-bit: a carry out of the low word
    big[1] += (1 << 32) - 3
    _run(dev, *a[:3], counts=big)
    assert big.tolist() == [(1 << 40) + int(a[3][0]), (1 << 40) + 5 + (1 << 32) - 3 + int(a[3][1])]


@pytest.mark.parametrize("B,A", ((3, 257), (1, LOOPS)))
def test_deterministic_mode_gives_the_same_counts(dev, B, A):
    from dan_amd import ops
    cls, labels, sel, want = case(B, A)
    plain = _run(dev, cls, labels, sel)
    with ops.use_context(ops.OpsContext(deterministic=True)):
        det = _run(dev, cls, labels, sel)
    assert torch.equal(plain, det) and np.array_equal(det.cpu().numpy(), want)


def test_selection_written_by_the_loss_is_what_the_metric_counts(dev):
    """sel as danhip_detection_loss_fwd writes it (0 / 1 mined negative / 2 positive): the metric through detection_loss(metric_counts=...)
    equals the restatement on that selection, and total equals the loss's own n_selected."""
    from dan_amd import ops
    B, A = 3, 515
    rng = np.random.RandomState(5)
    cls = torch.from_numpy(rng.randn(B, A, 2).astype(np.float32)).to(dev).requires_grad_()
    loc = torch.from_numpy(rng.randn(B, A, 4).astype(np.float32)).to(dev).requires_grad_()
    loc_t = torch.from_numpy(rng.randn(B, A, 4).astype(np.float32)).to(dev)
    labels = torch.from_numpy(rng.choice([-1, 0, 0, 0, 0, 0, 1], size=(B, A)).astype(np.int32)).to(dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    trace = {}
    with ops.use_context(ops.OpsContext(TRACE=trace)):
        acc = ops.detection_loss(cls, loc, labels, loc_t, metric_counts=counts)
    sel = trace["loss_sel"][0].cpu().numpy()
    want = reference(cls.detach().cpu().numpy(), labels.cpu().numpy(), sel)
    assert np.array_equal(counts.cpu().numpy(), want) and want[1] == int(acc[1].item()) > 0
