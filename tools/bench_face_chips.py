"""Face chips measured (no threshold is set; profiles/r24/face_chips.md keeps the result).

    python tools/bench_face_chips.py [--repeats 9] [--size 112] [--out FILE.json]

8 images 1024 wide with heights 576 .. 1536 and a fixed synthetic set of 40 detections per image (sides 16 .. 400 px, some leaving the
image), every row a chip.  Two arms on the same device tensors:
  extract    utility.face_chips.extract: two launches, nothing read back;
  per_chip   what the code had before: one download of (dets, num), the rule per row on the host, a slice of the image per chip made
             contiguous, and danhip_resize_u8_linear (eval_dan.resize_image) per chip.
A timed sample is ONE call between two torch.cuda.synchronize() on a host clock (the per_chip arm synchronises inside anyway); the arms
alternate inside every repeat in a rotating order; the figure is the median, the spread (min .. max) is printed with it.  The device time
of the two extract launches alone (device events around `launches` back-to-back calls) is reported beside it.  The first chips of the two
arms are compared first."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, HEIGHTS, ROWS = 1024, (576, 640, 768, 896, 1024, 1152, 1344, 1536), 40


def _inputs(dev):
    rng = np.random.RandomState(24)
    images = [torch.from_numpy(rng.randint(0, 256, (h, W, 3)).astype(np.uint8)).to(dev) for h in HEIGHTS]
    dets = np.zeros((len(HEIGHTS), ROWS, 5), np.float32)
    for i, h in enumerate(HEIGHTS):
        side = np.exp(rng.rand(ROWS) * np.log(400 / 16.0)) * 16
        x1, y1 = rng.rand(ROWS) * (W - 16), rng.rand(ROWS) * (h - 16)
        dets[i] = np.stack([x1, y1, x1 + side * 0.8, y1 + side, 0.2 + 0.8 * rng.rand(ROWS)], 1)
    return images, torch.from_numpy(dets).to(dev), torch.full((len(HEIGHTS),), ROWS, dtype=torch.int32, device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from dan_amd import eval_dan
    from dan_amd.utility import face_chips
    dev = torch.device("cuda:0")
    images, dets, num = _inputs(dev)
    S = args.size
    out = face_chips.extract(images, dets, num, size=S)                         # buffers made once, reused by every timed call
    buffers = tuple(out)

    def extract():
        return face_chips.extract(images, dets, num, size=S, out=buffers)

    def per_chip():
        host, counts = dets.cpu().numpy(), num.cpu().numpy()
        chips = []
        for i, image in enumerate(images):
            for r in range(int(counts[i])):
                rect = face_chips.rule(host[i, r], int(image.shape[0]), int(image.shape[1]), 0, True)
                if rect is not None and not host[i, r, 4] < np.float32(0.0):
                    crop = image[rect[1]:rect[3] + 1, rect[0]:rect[2] + 1]
                    chips.append(eval_dan.resize_image(crop, float(S) / crop.shape[1], float(S) / crop.shape[0]))
        return chips

    n = int(extract().count.item())
    old = per_chip()
    same = len(old) == n and all(torch.equal(old[k], buffers[0][k]) for k in range(0, n, 7))
    arms = {"extract": extract, "per_chip": per_chip}

    def sample(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    for fn in arms.values():
        sample(fn)
    times = {k: [] for k in arms}
    names = list(arms)
    for r in range(args.repeats):
        for k in range(len(names)):
            name = names[(k + r) % len(names)]
            times[name].append(sample(arms[name]))
    device_only = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            extract()
        b.record()
        b.synchronize()
        device_only.append(a.elapsed_time(b) / args.launches * 1e3)
    result = {"device": torch.cuda.get_device_name(0), "images": len(HEIGHTS), "width": W, "heights": list(HEIGHTS), "rows_per_image": ROWS,
              "size": S, "chips": n, "repeats": args.repeats, "arms_agree_on_every_7th_chip": bool(same)}
    for name, t in list(times.items()) + [("extract_back_to_back", device_only)]:
        result[name + "_us"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
        print("%s: median %.1f us (min %.1f, max %.1f)" % (name, statistics.median(t), min(t), max(t)))
    result["per_chip_over_extract"] = result["per_chip_us"]["median"] / result["extract_us"]["median"]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
