"""GPU suite of the WIDER FACE evaluator: dan_amd.wider_eval.WiderEvaluator (csrc/wider_eval_exact.hip) against the numpy restatement of
tests/wider_protocol.py.  Tolerances are derived, not measured: every decision of steps 1-4 compares doubles computed by the same IEEE
operations in the same order on both sides, so curves and count_face must be EQUAL; the AP is a sum of at most 1002 terms in [0, 1]
accumulated in the same order: 1e-12 absolute leaves a hundredfold margin over 1002 * 2^-53."""
import json
import os

import numpy as np
import pytest
import torch

import wider_protocol as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "wider_kats.json")))["kats"]
AP_TOL = 1e-12
BOUND = 2048                                                          # DANHIP_WIDER_MAX_DETS


def _gt(boxes, keep, subsets):
    from dan_amd.wider_eval import WiderGroundTruth
    return WiderGroundTruth(boxes, keep, subsets=subsets)


def _check(res, ref, subsets):
    assert np.array_equal(res["curves"], ref["curves"])
    assert np.array_equal(res["count_face"], ref["count_face"])
    for s, name in enumerate(subsets):
        assert abs(res[name] - ref["ap"][s]) <= AP_TOL, (name, res[name], ref["ap"][s])
    assert np.abs(res["precision"] - ref["precision"]).max() <= AP_TOL and np.abs(res["recall"] - ref["recall"]).max() <= AP_TOL
    assert res["score_range"] == (ref["lo"], ref["hi"])


def _reference(raw, boxes, keep, S, quantize):
    """The restatement on what the evaluator is defined to see: the raw rows, or (quantize) the rows read back from write_to_txt's text."""
    from dan_amd.eval_dan import write_to_txt
    dets = [W.text_route(write_to_txt, r, "ev", "im%d" % i) if quantize else np.asarray(r, dtype=np.float64).reshape(-1, 5) for i, r in enumerate(raw)]
    return W.evaluate(dets, boxes, keep, S), dets


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_known_answers(kat, dev):
    from dan_amd.wider_eval import WiderEvaluator
    S = kat["subsets"]
    subsets = tuple("s%d" % s for s in range(S))
    boxes = [np.asarray(im["boxes"], dtype=np.float64).reshape(-1, 4) for im in kat["images"]]
    keep = [np.asarray(im["keep"], dtype=np.uint8).reshape(len(b), S) for im, b in zip(kat["images"], boxes)]
    raw = [np.asarray(im["dets"], dtype=np.float32 if kat["quantize"] else np.float64).reshape(-1, 5) for im in kat["images"]]
    ev = WiderEvaluator(_gt(boxes, keep, subsets), quantize=kat["quantize"], max_per_image=16, device=dev)
    for i, r in enumerate(raw):
        ev.add_rows(i, torch.from_numpy(r))
    res = ev.result()
    exp = kat["expect"]
    want = np.zeros((S, 1000, 2), dtype=np.int64)
    for s, runs in enumerate(exp["curve_runs"]):
        for a, b, c0, c1 in runs:
            want[s, a:b + 1] = (c0, c1)
    assert np.array_equal(res["curves"], want)
    assert res["count_face"].tolist() == exp["count_face"]
    for s, name in enumerate(subsets):
        assert abs(res[name] - exp["ap"][s]) <= AP_TOL
    assert res["score_range"] == (exp["lo"], exp["hi"])
    ref, _ = _reference(raw, boxes, keep, S, kat["quantize"])
    _check(res, ref, subsets)
    zero = res["curves"][..., 0] == 0                                 # 0 / 0 is 0 by definition, and only ever where nothing was recalled
    assert (res["precision"][zero] == 0).all() and (res["curves"][..., 1][zero] == 0).all()


def make_set(seed, quantize):
    """A seeded set with everything the protocol branches on: boxes kept in none / some / all of three nested subsets, duplicate detections of
    a box, images without boxes, without detections, with detections that all fall to the text filters, heavy score ties (a 1/16 grid, or
    the 1/1000 grid of the text), one image with more boxes than an LDS tile (512) holds and one with detections at the kernel's bound.
    -> (raw rows per image, boxes, keep); raw rows are fp32 (xmin, ymin, xmax, ymax, score) when quantize, else float64 (x, y, w, h, score)."""
    rng = np.random.RandomState(1000 + seed)
    I = int(rng.randint(40, 90))
    raw, boxes, keep = [], [], []
    for i in range(I):
        kind = {3: "many_boxes", 5: "bound", 7: "no_boxes", 9: "no_dets", 11: "filtered"}.get(i) or str(rng.choice(["plain"] * 6 + ["no_boxes", "no_dets", "filtered"]))
        m = 600 if kind == "many_boxes" else 0 if kind == "no_boxes" else int(rng.randint(1, 9))
        wh = rng.randint(12, 80, (m, 2))
        xy = rng.randint(0, 900, (m, 2))
        b = np.concatenate([xy, wh], axis=1).astype(np.float64)
        level = rng.randint(0, 4, m)                                  # 0: kept nowhere; 1: hard; 2: medium + hard; 3: all
        k = np.stack([level >= 3, level >= 2, level >= 1], axis=1).astype(np.uint8)
        rows = []
        for j in range(m):                                            # 0-3 detections per box, close enough to match: duplicates
            for _ in range(int(rng.randint(0, 4)) if kind != "many_boxes" else int(rng.rand() < 0.1)):
                jit = rng.randn(4) * 0.04 * b[j, 2:].min()
                rows.append([b[j, 0] + jit[0], b[j, 1] + jit[1], max(2.0, b[j, 2] + jit[2]), max(10.0, b[j, 3] + jit[3])])
        n_noise = BOUND - len(rows) if kind == "bound" else int(rng.randint(0, 30))
        for _ in range(n_noise):
            rows.append([rng.rand() * 900, rng.rand() * 900, 12 + rng.rand() * 60, 12 + rng.rand() * 60])
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 4)
        if kind == "no_dets":
            rows = rows[:0]
        if kind == "filtered":                                        # every row too low for the text route (height below 10)
            rows[:, 3] = 4.0
        rows = rows[rng.permutation(len(rows))]
        if quantize:
            score = rng.randint(11, 1000, len(rows)) / 1000.0 if seed % 2 else 0.011 + rng.rand(len(rows)) * 0.98
            r = np.concatenate([rows[:, :2], rows[:, :2] + rows[:, 2:] - 1, score[:, None]], axis=1).astype(np.float32)
            r[::7, 4] = 0.005                                         # under the score filter
        else:
            score = rng.randint(1, 17, len(rows)) / 16.0
            r = np.concatenate([rows, score[:, None]], axis=1)
        raw.append(r)
        boxes.append(b)
        keep.append(k)
    return raw, boxes, keep


def feed(ev, raw, order, batch, dev, device_index=False, skip_empty=False):
    """Adds the images in `order`, `batch` at a time, as padded [B, Nmax, 5] blocks whose rows beyond num are rubbish."""
    dtype = torch.float32 if raw[0].dtype == np.float32 else torch.float64
    for p in range(0, len(order), batch):
        idx = [i for i in order[p:p + batch] if not (skip_empty and len(raw[i]) == 0)]
        if not idx:
            continue
        nmax = max(1, max(len(raw[i]) for i in idx))
        block = torch.full((len(idx), nmax, 5), 1.0e6, dtype=dtype)
        for b, i in enumerate(idx):
            block[b, :len(raw[i])] = torch.from_numpy(raw[i])
        num = torch.tensor([len(raw[i]) for i in idx], dtype=torch.int32)
        ev.add(torch.tensor(idx, dtype=torch.int64, device=dev) if device_index else idx, block.to(dev), num.to(dev))


@pytest.mark.parametrize("quantize", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_synthetic_sets_match_the_restatement_whatever_the_batching(seed, quantize, dev):
    from dan_amd.wider_eval import WiderEvaluator
    subsets = ("easy", "medium", "hard")
    raw, boxes, keep = make_set(seed, quantize)
    ref, dets = _reference(raw, boxes, keep, 3, quantize)
    n_after = [len(d) for d in dets]
    assert max(n_after) > 1500 and min(n_after) == 0 and max(len(b) for b in boxes) > 512 and min(len(b) for b in boxes) == 0
    assert ref["curves"][..., 1].max() > 10 and (ref["count_face"] > 0).all()
    if quantize:
        assert any(len(r) > 0 and n == 0 for r, n in zip(raw, n_after))           # an image emptied by the filters
    gt = _gt(boxes, keep, subsets)
    I = len(raw)
    results = []
    plans = [(list(range(I)), 8, False, False), (list(np.random.RandomState(seed).permutation(I)), 3, True, False),
             (list(range(I))[::-1], 1 if I < 50 else 5, False, True), (list(range(I)), 8, False, False)]
    for order, batch, device_index, skip_empty in plans:
        ev = WiderEvaluator(gt, quantize=quantize, max_per_image=BOUND, device=dev)
        feed(ev, raw, [int(i) for i in order], batch, dev, device_index, skip_empty)
        results.append(ev.result())
    _check(results[0], ref, subsets)
    for r in results[1:]:                                             # other batchings / image orders / a second run: the same bits
        assert np.array_equal(r["curves"], results[0]["curves"]) and np.array_equal(r["count_face"], results[0]["count_face"])
        assert all(r[name] == results[0][name] for name in subsets)
        assert np.array_equal(r["precision"], results[0]["precision"]) and np.array_equal(r["recall"], results[0]["recall"])


def test_text_files_and_raw_tensors_give_the_same_curves(tmp_path, dev):
    """write_to_txt -> files -> read_pred_dir -> restatement  ==  WiderEvaluator(quantize=True) fed the raw fp32 tensors."""
    from dan_amd import wider_eval
    from dan_amd.eval_dan import write_to_txt
    subsets = ("easy", "medium", "hard")
    raw, boxes, keep = make_set(11, True)
    names = ["%d--Event/%d_Event_img_%d" % (i % 4, i % 4, i) for i in range(len(raw))]
    for name, r in zip(names, raw):
        event, im = name.split("/")
        os.makedirs(tmp_path / event, exist_ok=True)
        with open(tmp_path / event / (im + ".txt"), "w") as f:
            write_to_txt(f, torch.from_numpy(r).to(dev), event, im)
    pred = wider_eval.read_pred_dir(str(tmp_path))
    assert sorted(pred) == sorted(names)
    ref = W.evaluate([pred[n] for n in names], boxes, keep, 3)
    gt = wider_eval.WiderGroundTruth(boxes, keep, names=names)
    ev = wider_eval.WiderEvaluator(gt, quantize=True, max_per_image=BOUND, device=dev)
    feed(ev, raw, list(range(len(raw))), 8, dev)
    res = ev.result()
    _check(res, ref, subsets)
    # and the parsed rows through the quantize=False door give the same again
    ev2 = wider_eval.WiderEvaluator(gt, quantize=False, max_per_image=BOUND, device=dev)
    for n in names:
        ev2.add_rows(gt.index_of(n), torch.from_numpy(pred[n]))
    res2 = ev2.result()
    assert np.array_equal(res2["curves"], res["curves"]) and all(res2[s] == res[s] for s in subsets)


def test_an_image_added_twice_raises(dev):
    from dan_amd.wider_eval import WiderEvaluator
    gt = _gt([np.array([[0, 0, 9, 9]]), np.array([[5, 5, 20, 20]])], [np.array([[1]]), np.array([[1]])], ("all",))
    rows = torch.tensor([[0.0, 0.0, 9.0, 9.0, 0.5]], dtype=torch.float64)
    ev = WiderEvaluator(gt, quantize=False, max_per_image=8, device=dev)
    ev.add_rows(0, rows)
    with pytest.raises(ValueError):
        ev.add_rows(0, rows)
    ev = WiderEvaluator(gt, quantize=False, max_per_image=8, device=dev)      # indices on the device: found by the kernel, reported by result()
    idx = torch.tensor([1], dtype=torch.int32, device=dev)
    num = torch.tensor([1], dtype=torch.int32, device=dev)
    ev.add(idx, rows.reshape(1, 1, 5).to(dev), num)
    ev.add(idx, rows.reshape(1, 1, 5).to(dev), num)
    with pytest.raises(ValueError, match="twice"):
        ev.result()
    ev = WiderEvaluator(gt, quantize=False, max_per_image=8, device=dev)
    ev.add(torch.tensor([7], dtype=torch.int32, device=dev), rows.reshape(1, 1, 5).to(dev), num)
    with pytest.raises(ValueError, match="outside"):
        ev.result()


def _fake_net_np(image):
    """The deterministic stand-in network of the test-time pipeline's tests: boxes / scores derived from the image content with integer
    arithmetic only; twelve "faces" collect many hits each."""
    h, w = image.shape[:2]
    key = (int(image.astype(np.int64).sum()) + 7919 * h + 104729 * w) % (2 ** 31 - 1)
    rng = np.random.RandomState(key)
    n = 1500
    cy, cx = rng.rand(n) * h, rng.rand(n) * w
    s = np.exp(rng.rand(n) * np.log(40)) * 6
    face = rng.randint(0, 12, n)
    fy, fx, fs = _faces(h, w)
    hit = rng.rand(n) < 0.5
    cy = np.where(hit, fy[face] + rng.randn(n) * fs[face] * 0.05, cy)
    cx = np.where(hit, fx[face] + rng.randn(n) * fs[face] * 0.05, cx)
    s = np.where(hit, fs[face] * (1 + rng.randn(n) * 0.05), s)
    boxes = np.stack([cy - s / 2, cx - s / 2, cy + s / 2, cx + s / 2], 1).astype(np.float32)
    scores = np.where(hit, 0.5 + rng.rand(n) * 0.5, rng.rand(n) * 0.3).astype(np.float32)
    return boxes, scores


def _faces(h, w):
    return (np.arange(12) * 37 % 11 + 1) / 12.0 * h, (np.arange(12) * 53 % 11 + 1) / 12.0 * w, (np.arange(12) % 4 + 1) * 0.06 * min(h, w)


class _FakeBatchNet(object):
    def __call__(self, image):
        b, s = _fake_net_np(image.cpu().numpy())
        return torch.from_numpy(b).to(image.device), torch.from_numpy(s).to(image.device)

    def batch(self, images):
        outs = [self(images[b]) for b in range(images.shape[0])]
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


def test_end_to_end_from_images_to_ap(tmp_path, dev):
    """stand-in network -> detect_images -> add -> result, against the restatement run on the text files of the same detections."""
    from dan_amd import eval_dan as P
    from dan_amd import wider_eval
    h, w = 240, 320
    rng = np.random.RandomState(77)
    imgs = torch.from_numpy(rng.randint(0, 256, (4, h, w, 3)).astype(np.uint8)).to(dev)
    fy, fx, fs = _faces(h, w)
    box = np.stack([np.floor(fx - fs / 2), np.floor(fy - fs / 2), np.ceil(fs), np.ceil(fs)], axis=1)
    boxes = [box, box[:7], box[3:], np.zeros((0, 4))]
    level = np.arange(12) % 4
    k = np.stack([level >= 3, level >= 2, level >= 1], axis=1).astype(np.uint8)
    keep = [k, k[:7], k[3:], k[:0]]
    names = ["0--Event/img_%d" % i for i in range(4)]
    gt = wider_eval.WiderGroundTruth(boxes, keep, names=names)
    ev = wider_eval.WiderEvaluator(gt, device=dev)                    # the defaults: quantize, 750 rows per image
    net = _FakeBatchNet()
    os.makedirs(tmp_path / "0--Event")
    for first in (0, 2):
        dets, num = P.detect_images(net, imgs[first:first + 2], pyramid=False)
        ev.add([first, first + 1], dets, num)
        for b in range(2):
            with open(tmp_path / "0--Event" / ("img_%d.txt" % (first + b)), "w") as f:
                P.write_to_txt(f, dets[b, :int(num[b].item())], "0--Event", "img_%d" % (first + b))
    res = ev.result()
    pred = wider_eval.read_pred_dir(str(tmp_path))
    ref = W.evaluate([pred[n] for n in names], boxes, keep, 3)
    _check(res, ref, gt.subsets)
    assert res["curves"][..., 1].max() >= 5 and 0 < res["hard"] <= 1   # the stand-in's faces are found: the comparison is not of zeros
