"""Times the on-device WIDER FACE evaluator (dan_amd/wider_eval.py) on a seeded synthetic set of validation size and the numpy restatement
(tests/wider_protocol.py) on the same set on the host.

    python tools/bench_wider_eval.py [--images 3226] [--repeats 10] [--no-host] [--out FILE.md]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_wider_eval.py --images N --trace-only      # launches of ONE result()

The set: a long-tailed number of boxes per image (about 39.7 k boxes over 3226 images, up to about 1000 in one), up to 750 fp32 detections per
image as detect_images returns them ([8, 750, 5] blocks + counts), three nested subsets.  add() is timed per batch of 8 with device events
(median over the batches of each repeat), result() alone with events around it (it ends in its own read-back), median of the repeats after
one warm-up.  Needs a GPU: there is no fallback."""
import argparse
import os
import socket
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from dan_amd import wider_eval                                       # noqa: E402

CAP, BATCH = 750, 8


def make_set(images, seed=0):
    rng = np.random.RandomState(seed)
    m = np.minimum(1900, np.floor(np.exp(rng.randn(images) * 1.35 + 1.75))).astype(np.int64)       # long tail: median ~4, mean ~12
    m[rng.rand(images) < 0.02] = 0
    boxes, keep, raw = [], [], []
    for i in range(images):
        wh = np.floor(np.exp(rng.rand(m[i], 2) * 2.6 + 2.3))
        xy = rng.randint(0, 1000, (m[i], 2))
        b = np.concatenate([xy, wh], axis=1).astype(np.float64)
        level = rng.randint(0, 4, m[i])
        boxes.append(b)
        keep.append(np.stack([level >= 3, level >= 2, level >= 1], axis=1).astype(np.uint8))
        hits = b[rng.rand(m[i]) < 0.8]
        hits = np.repeat(hits, rng.randint(1, 3, len(hits)), axis=0)
        hits = hits + rng.randn(*hits.shape) * 0.05 * hits[:, 2:].min(axis=1, keepdims=True)
        n_noise = int(min(CAP - min(len(hits), CAP), np.floor(np.exp(rng.rand() * 6.6))))
        noise = np.concatenate([rng.rand(n_noise, 2) * 1000, 8 + rng.rand(n_noise, 2) * 80], axis=1)
        rows = np.concatenate([hits, noise], axis=0)[:CAP]
        score = np.concatenate([0.3 + 0.7 * rng.rand(len(hits)), rng.rand(n_noise) ** 2])[:CAP]
        r = np.concatenate([rows[:, :2], rows[:, :2] + np.maximum(rows[:, 2:], 1) - 1, score[:, None]], axis=1).astype(np.float32)
        raw.append(r[rng.permutation(len(r))])
    return raw, boxes, keep


def blocks(raw, dev):
    out = []
    for p in range(0, len(raw), BATCH):
        idx = list(range(p, min(p + BATCH, len(raw))))
        block = torch.zeros((len(idx), CAP, 5), dtype=torch.float32)
        for b, i in enumerate(idx):
            block[b, :len(raw[i])] = torch.from_numpy(raw[i])
        out.append((torch.tensor(idx, dtype=torch.int32, device=dev), block.to(dev), torch.tensor([len(raw[i]) for i in idx], dtype=torch.int32, device=dev)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=3226)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--trace-only", action="store_true", help="fill one evaluator, call result() once (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wider_eval needs a GPU")
    dev = torch.device("cuda:0")
    raw, boxes, keep = make_set(a.images)
    gt = wider_eval.WiderGroundTruth(boxes, keep)
    data = blocks(raw, dev)
    n_boxes, n_dets = int(gt.boxes.shape[0]), sum(len(r) for r in raw)

    def fill(timed):
        ev = wider_eval.WiderEvaluator(gt, max_per_image=CAP, device=dev)
        times = []
        for idx, block, num in data:                                  # indices on the device: add() has nothing to look at on the host
            if timed:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            ev.add(idx, block, num)
            if timed:
                e1.record()
                times.append((e0, e1))
        torch.cuda.synchronize()
        return ev, [e0.elapsed_time(e1) for e0, e1 in times]

    if a.trace_only:
        ev, _ = fill(False)
        res = ev.result()
        print("images %d boxes %d detections %d  AP %s" % (a.images, n_boxes, n_dets, [round(res[s], 6) for s in gt.subsets]))
        return
    fill(False)[0].result()                                           # warm-up: code objects, allocator
    add_ms, result_ms, res = [], [], None
    for _ in range(a.repeats):
        ev, t = fill(True)
        add_ms.append(statistics.median(t))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = ev.result()
        e1.record()
        torch.cuda.synchronize()
        result_ms.append(e0.elapsed_time(e1))
    lines = ["images %d, boxes %d (most in one image %d), detections in %d, three subsets, T = 1000" % (a.images, n_boxes, max(len(b) for b in boxes), n_dets),
             "box: %s, %s, torch %s" % (socket.gethostname(), torch.cuda.get_device_name(0), torch.__version__),
             "add(), one batch of %d x %d rows: median %.3f ms (median over the batches, then over %d repeats; min %.3f max %.3f)"
             % (BATCH, CAP, statistics.median(add_ms), a.repeats, min(add_ms), max(add_ms)),
             "result(): median %.3f ms over %d repeats (min %.3f max %.3f)" % (statistics.median(result_ms), a.repeats, min(result_ms), max(result_ms)),
             "AP: " + ", ".join("%s %.6f" % (s, res[s]) for s in gt.subsets)]
    if not a.no_host:
        import wider_protocol as W
        from dan_amd.eval_dan import write_to_txt
        t0 = time.time()
        dets = [W.text_route(write_to_txt, r) for r in raw]
        t1 = time.time()
        ref = W.evaluate(dets, boxes, keep, 3)
        t2 = time.time()
        same = bool(np.array_equal(ref["curves"], res["curves"])) and max(abs(ref["ap"][s] - res[n]) for s, n in enumerate(gt.subsets)) <= 1e-12
        dev_s = (statistics.median(add_ms) * len(data) + statistics.median(result_ms)) / 1e3
        lines += ["numpy restatement on the host, once, single thread: text route %.1f s + evaluation %.1f s; curves equal and AP within 1e-12: %s" % (t1 - t0, t2 - t1, same),
                  "ratio host evaluation / device (all add() calls + result()): %.0f x   (device total %.3f s)" % ((t2 - t1) / dev_s, dev_s)]
        if not same:
            lines.append("MISMATCH against the restatement")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if lines[-1].startswith("MISMATCH"):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
