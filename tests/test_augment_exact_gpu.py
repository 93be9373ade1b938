"""The training input pass (dan_amd/csrc/augment_exact.hip: danhip_augment_preprocess and danhip_augment_preprocess_batch) against the oracle
chain by EQUALITY (tests/augment_exact.py says why equality is the right check, and holds the cases; tests/test_augment_exact_cpu.py asserts
their preconditions): a palette of designed pixels under every colour op at the ends of its range, designed windows and output shapes, the
sizes at which the grid-stride loops and the capped mean reduction take another trip, bit-identity of the three forms of a pinned contrast
mean, and independence from what the output and the workspace held before."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_exact as AE  # noqa: E402

pytestmark = pytest.mark.gpu


def _P():
    from dan_amd.preprocessing import dan_preprocessing as P
    return P


def test_palette_under_every_chain_both_entry_points(dev):
    assert AE.run_palette(dev) == 2 * len(AE.PALETTE_CHAINS)


@pytest.mark.parametrize("out_shape", AE.GEOMETRY_OUT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_geometry_per_image(out_shape, dev):
    assert AE.run_geometry(out_shape, dev, batch=False) == len(AE.GEOMETRY_WINDOWS) * 2 * 2


@pytest.mark.parametrize("out_shape", AE.GEOMETRY_OUT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_geometry_batch_with_the_window_flip(out_shape, dev):
    assert AE.run_geometry(out_shape, dev, per_image=False) == len(AE.GEOMETRY_WINDOWS) * 3 * 2


@pytest.mark.parametrize("name", ["output_second_trip", "mean_second_trip"])
def test_looping_sizes_per_image(name, dev):
    src, ops, win, out_shape = AE.LOOPING[name]
    img = AE.noisy_image(*src)
    got = _P().augment_image(torch.from_numpy(img).to(dev), ops, win, False, out_shape)
    AE.assert_exact(got, AE.oracle(img, ops, win, 0, out_shape), name)


def test_looping_batch_mean_above_the_workgroup_cap(dev):
    images, items = AE.looping_batch()
    out = _P().augment_batch([torch.from_numpy(a).to(dev) for a in images], items, AE.LOOPING_BATCH_OUT)
    for k, (img, (ops, win, flip)) in enumerate(zip(images, items)):
        AE.assert_exact(out[k], AE.oracle(img, ops, win, flip, AE.LOOPING_BATCH_OUT), "looping batch item %d" % k)


def test_pinned_contrast_means_three_forms_bit_identical(dev):
    """Contrast first (every partial sum exact) and contrast later on inputs whose sums are order-independent: the batch slice, the
    per-image result and the oracle are one and the same tensor."""
    P = _P()
    cases = list(AE.CONTRAST_FIRST.items()) + list(AE.CONTRAST_LATER.items())
    hosts = [AE.noisy_image(*src) for _, (src, _, _, _) in cases]
    imgs = [torch.from_numpy(a).to(dev) for a in hosts]
    out = P.augment_batch(imgs, [(ops, win, flip) for _, (_, ops, win, flip) in cases], AE.CONTRAST_OUT)
    for k, (name, (_, ops, win, flip)) in enumerate(cases):
        single = P.augment_image(imgs[k], ops, win, bool(flip), AE.CONTRAST_OUT)
        assert torch.equal(out[k], single), name
        ref = torch.zeros_like(single)
        ref[..., :3] = torch.from_numpy(AE.oracle(hosts[k], ops, win, flip, AE.CONTRAST_OUT)).to(single.dtype)
        assert torch.equal(single, ref), name
        AE.assert_exact(out[k], AE.oracle(hosts[k], ops, win, flip, AE.CONTRAST_OUT), name)


def test_result_does_not_depend_on_what_output_and_workspace_held(dev):
    """The library zero-fills the sums of the contrast mean itself and writes every output element: a NaN pattern in both changes nothing."""
    import ctypes
    from dan_amd._lib import ACT_DTYPE, call, lib, ptr, stream
    P = _P()
    hosts, (_, items, (oh, ow)) = AE.isolation_images(), AE.ISOLATION
    imgs = [torch.from_numpy(a).to(dev) for a in hosts]
    # per image: the library call of dan_preprocessing.augment_image on buffers that hold NaN patterns
    ops, win, flip = items[0]
    want = P.augment_image(imgs[0], ops, win, flip, (oh, ow))
    AE.assert_exact(want, AE.oracle(hosts[0], ops, win, flip, (oh, ow)), "per image")
    nws = lib().danhip_augment_workspace_bytes()
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.full((oh, ow, 8), float("nan"), dtype=ACT_DTYPE, device=dev)
    codes = (ctypes.c_int32 * 4)(*([P.OP_CODES[n] for n, _ in ops] + [0] * (4 - len(ops))))
    vals = (ctypes.c_float * 4)(*([float(v) for _, v in ops] + [0.0] * (4 - len(ops))))
    call("danhip_augment_preprocess", ptr(imgs[0]), int(hosts[0].shape[0]), int(hosts[0].shape[1]), len(ops), codes, vals, win[0], win[1], win[2], win[3],
         int(flip), ptr(out), oh, ow, ptr(ws), nws, stream())
    assert torch.equal(out, want)
    # batch: the table of the call just made is still on the device; the same library call on NaN-filled output and workspace
    first = P.augment_batch(imgs, items, (oh, ow)).clone()
    for k, (a, (ops, win, flip)) in enumerate(zip(hosts, items)):
        AE.assert_exact(first[k], AE.oracle(a, ops, win, flip, (oh, ow)), "batch item %d" % k)
    table, ws = P._batch_buffers(dev, len(imgs))[2:4]
    ws.fill_(0xFF)
    out = torch.full((len(imgs), oh, ow, 8), float("nan"), dtype=ACT_DTYPE, device=dev)
    total = sum(AE.mean_blocks(a.shape[0], a.shape[1], ops) for a, (ops, _, _) in zip(hosts, items))
    assert total == 4 + 0 + 3                                                     # ceil(6300 / 2048), none, ceil(4950 / 2048)
    call("danhip_augment_preprocess_batch", ptr(table), len(imgs), total, ptr(out), oh, ow, ptr(ws), ws.numel(), stream())
    assert torch.equal(out, first)
