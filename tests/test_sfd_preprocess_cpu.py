"""The window and box half of dan_amd/preprocessing/sfd_preprocessing.py (no device needed): hand-traced known answers
(tests/golden/sfd_preprocess_kats.json), a loop-by-loop restatement of the reference's lines (tests/sfd_preprocess_loop.py) over 200 seeded
images, and the renamed surface of pb_preprocessing.py."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sfd_preprocess_loop as L  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(HERE, "golden", "sfd_preprocess_kats.json")) as f:
        return json.load(f)


def _boxes_equal(got, want):
    got, want = np.asarray(got, F).reshape(-1, 4), np.asarray(want, F).reshape(-1, 4)
    return got.shape == want.shape and np.array_equal(got, want)


def test_patch_wrapper_known_answers(kats):
    from dan_amd.preprocessing import sfd_preprocessing as S
    names = [k["name"] for k in kats["patch_wrapper"]]
    assert len(names) >= 4 and any("first" in n for n in names) and any("25 attempts" in n for n in names) \
        and any("edge" in n and "strict" in n for n in names) and any("1.0" in n for n in names)
    for k in kats["patch_wrapper"]:
        for fn in (S.sfd_random_sample_patch_wrapper, L.patch_wrapper_loop):          # the module, and the restatement it is compared with below
            d = L.ScriptedDraws(k["draws"])
            win, boxes = fn(k["height"], k["width"], np.asarray(k["bboxes"], F), d)
            assert d.done(), (k["name"], "draws left over")
            assert tuple(int(v) for v in win) == tuple(k["window"]), (k["name"], win)
            assert _boxes_equal(boxes, k["boxes"]), (k["name"], boxes)


def test_train_known_answers(kats):
    from dan_amd.preprocessing import sfd_preprocessing as S
    for k in kats["train"]:
        for fn in (S.draw_for_train, L.draw_for_train_loop):
            d = L.ScriptedDraws(k["draws"])
            ops, win, flip, boxes = fn(k["height"], k["width"], np.asarray(k["bboxes"], F), k["out_shape"], d)
            assert d.done(), (k["name"], "draws left over")
            assert [[n, float(v)] for n, v in ops] == k["ops"], k["name"]
            assert tuple(int(v) for v in win) == tuple(k["window"]) and bool(flip) == k["flip"], (k["name"], win, flip)
            assert _boxes_equal(boxes, k["boxes"]), (k["name"], boxes)


def _seeded_case(seed):
    rng = np.random.RandomState(seed)
    h, w = int(rng.randint(40, 700)), int(rng.randint(40, 900))
    n = int(rng.randint(1, 9))
    cy, cx = rng.rand(n) * h, rng.rand(n) * w
    s = np.exp(rng.rand(n) * np.log(12)) * 6
    if seed % 5 == 0:                                                             # faces in one corner: the 25 attempts often all miss
        cy, cx = cy * 0.04, cx * 0.04
    b = np.stack([np.clip(cy - s / 2, 0, h - 1), np.clip(cx - s / 2, 0, w - 1), np.clip(cy + s / 2, 0, h - 1), np.clip(cx + s / 2, 0, w - 1)], 1)
    out_shape = [(640, 640), (160, 96), (300, 300)][seed % 3]
    return h, w, b.astype(F), out_shape


def test_module_equals_the_loop_restatement_over_200_images():
    from dan_amd.preprocessing import sfd_preprocessing as S
    flips = 0
    for seed in range(200):
        h, w, b, out_shape = _seeded_case(seed)
        win_a, boxes_a = S.sfd_random_sample_patch_wrapper(h, w, b, S.Draws(1000 + seed))
        win_b, boxes_b = L.patch_wrapper_loop(h, w, b, S.Draws(1000 + seed))
        assert tuple(win_a) == tuple(win_b) and _boxes_equal(boxes_a, boxes_b), seed
        da, db = S.Draws(2000 + seed), S.Draws(2000 + seed)
        ops_a, win_a, flip_a, boxes_a = S.draw_for_train(h, w, b, out_shape, da)
        ops_b, win_b, flip_b, boxes_b = L.draw_for_train_loop(h, w, b, out_shape, db)
        assert [(n, float(v)) for n, v in ops_a] == [(n, float(v)) for n, v in ops_b], seed
        assert tuple(win_a) == tuple(win_b) and flip_a == flip_b and _boxes_equal(boxes_a, boxes_b), seed
        assert da.r.random_sample() == db.r.random_sample(), seed                 # the same number of draws was taken
        flips += int(flip_a)
    assert 40 < flips < 160                                                       # both branches of the flip were compared


def test_pb_names_resolve_to_the_dan_functions():
    from dan_amd.preprocessing import dan_preprocessing as D
    from dan_amd.preprocessing import pb_preprocessing as P
    for name in ("distort_color", "pyramid_box_random_sample_patch_wrapper", "data_anchor_sampling", "random_flip_left_right",
                 "preprocess_for_train", "preprocess_batch_for_train"):
        assert getattr(P, name) is getattr(D, name)
    assert not hasattr(P, "dan_random_sample") and not hasattr(P, "dan_random_sample_patch_wrapper")
    for seed in range(20):
        h, w, b, out_shape = _seeded_case(300 + seed)
        win_a, boxes_a = P.sfd_random_sample_patch_wrapper(h, w, b, P.Draws(seed))
        win_b, boxes_b = D.dan_random_sample_patch_wrapper(h, w, b, D.Draws(seed))
        assert tuple(win_a) == tuple(win_b) and _boxes_equal(boxes_a, boxes_b), seed
        win_a, boxes_a = P.sfd_random_sample(h, w, b, out_shape, P.Draws(seed))
        win_b, boxes_b = D.dan_random_sample(h, w, b, out_shape, D.Draws(seed))
        assert tuple(win_a) == tuple(win_b) and _boxes_equal(boxes_a, boxes_b), seed


def test_item_helper_validates_what_it_is_given():
    """danhip_augment_item_init is host code: more than four ops, two contrast ops, an unknown op code and a non-positive window are refused."""
    import ctypes
    from dan_amd import _lib
    lib = _lib.lib()
    assert lib.danhip_version() >= 11
    item = ctypes.create_string_buffer(lib.danhip_augment_item_bytes())
    src = ctypes.create_string_buffer(16)                                         # never read: the helper only records the address
    nb = ctypes.c_int32(-1)

    def init(codes, window=(0, 0, 4, 4), h=2, w=2, flip=0):
        c = (ctypes.c_int32 * 8)(*(list(codes) + [0] * (8 - len(codes))))
        v = (ctypes.c_float * 8)(*([1.0] * 8))
        return lib.danhip_augment_item_init(ctypes.addressof(item), ctypes.addressof(src), h, w, len(codes), c, v, window[0], window[1], window[2],
                                            window[3], flip, 0, ctypes.byref(nb))

    assert init([]) == 0 and nb.value == 0
    assert init([0, 1, 2]) == 0 and nb.value == 0                                 # no contrast op: no workgroup of the mean launch
    assert init([0, 1, 2, 3]) == 0 and nb.value == 1
    assert init([3], h=2000, w=3000) == 0 and 1 < nb.value <= 2000 * 3000 // 256
    assert init([0, 1, 2, 3, 0]) == -1 and b"4" in lib.danhip_last_error()
    assert init([3, 0, 3]) == -1 and init([4]) == -1 and init([-1]) == -1
    assert init([], window=(0, 0, 0, 4)) == -1 and init([], window=(0, 0, 4, -1)) == -1
    assert init([], window=(-5, -7, 4, 4)) == 0                                   # the window may leave the image
    assert init([], flip=3) == -1 and init([], flip=2) == 0
    assert lib.danhip_augment_batch_workspace_bytes(0) == 0 and lib.danhip_augment_batch_workspace_bytes(17) >= 17 * 24
    # host-checked arguments of the batched call itself (nothing is launched)
    assert lib.danhip_augment_preprocess_batch(None, 1, 0, ctypes.addressof(src), 8, 8, ctypes.addressof(src), 64, None) == -1
    assert lib.danhip_augment_preprocess_batch(ctypes.addressof(item), 0, 0, ctypes.addressof(src), 8, 8, ctypes.addressof(src), 64, None) == -1
    assert lib.danhip_augment_preprocess_batch(ctypes.addressof(item), 1, 0, ctypes.addressof(src), 0, 8, ctypes.addressof(src), 64, None) == -1
    assert lib.danhip_augment_preprocess_batch(ctypes.addressof(item), 1, 0, ctypes.addressof(src), 8, -1, ctypes.addressof(src), 64, None) == -1
