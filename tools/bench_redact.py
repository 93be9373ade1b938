"""Face redaction measured (no threshold is set; profiles/r26/redact.md keeps the result).

    python tools/bench_redact.py [--repeats 9] [--launches 20] [--out FILE.json]

The r24 set: 8 images 1024 wide with heights 576 .. 1536 and 40 synthetic detections per image (sides 16 .. 400 px, "small"), and the
same images with 40 detections per image 300 .. 600 px wide (320 in all, "large").  On the same device tensors:
  redact/<mode>/<shape>   utility.redact.apply at the default strength into buffers made once: three launches, nothing read back;
  copy                    a plain device copy of the same images (torch's copy_ per image): the floor - the call reads and writes every
                          image once;
  draw                    draw_toolbox.bboxes_draw_on_img_list (in place) on the same boxes;
  host                    what a user had before: download images and detections, per box a numpy box filter from a summed-area
                          table (the same rule: windows clipped to the image, round half up), upload.  Timed on the large set with 3 repeats.
  blur/fixed/e=4,32,255   320 large boxes blurred with the extent forced through `strength`: e = longer side * strength, so the boxes of
                          these arms are all 400 x 500 and the strengths 4 / 500, 32 / 500 and 1.
A timed sample is `launches` back-to-back calls between two device events (the median over `repeats` samples, min .. max beside it); the
arms alternate inside every repeat in a rotating order.  The redacted bytes of one arm are compared with the host path's first."""
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
    sets = {}
    for name in ("small", "large", "fixed"):
        dets = np.zeros((len(HEIGHTS), ROWS, 5), np.float32)
        for i, h in enumerate(HEIGHTS):
            if name == "small":
                side = np.exp(rng.rand(ROWS) * np.log(400 / 16.0)) * 16
                w, hh = side * 0.8, side
            elif name == "large":
                w = 300 + rng.rand(ROWS) * 300
                hh = w * 1.25
            else:
                w, hh = np.full(ROWS, 399.0), np.full(ROWS, 499.0)       # 400 x 500 after the +1
            x1, y1 = rng.rand(ROWS) * (W - w), rng.rand(ROWS) * np.maximum(h - hh, 1)
            dets[i] = np.stack([x1, y1, x1 + w, y1 + hh, 0.2 + 0.8 * rng.rand(ROWS)], 1)
        sets[name] = torch.from_numpy(dets).to(dev)
    return images, sets, torch.full((len(HEIGHTS),), ROWS, dtype=torch.int32, device=dev)


def host_blur(images, dets, num, strength_pm=125):
    """download, per-box box filter from a summed-area table, upload"""
    from dan_amd.utility import redact
    rows, counts = dets.cpu().numpy(), num.cpu().numpy()
    out = []
    for i, image in enumerate(images):
        im = image.cpu().numpy()
        H, Wd = im.shape[:2]
        sat = np.zeros((H + 1, Wd + 1, 3), np.int64)
        sat[1:, 1:] = im.astype(np.int64).cumsum(0).cumsum(1)
        res = im.copy()
        for r, rect, e in redact.valid_rows(rows[i], H, Wd, int(counts[i]), strength_pm):
            x1, y1, x2, y2 = rect
            ys, xs = np.arange(y1, y2 + 1), np.arange(x1, x2 + 1)
            y0, y3 = np.maximum(ys - e, 0), np.minimum(ys + e, H - 1) + 1
            x0, x3 = np.maximum(xs - e, 0), np.minimum(xs + e, Wd - 1) + 1
            S = sat[y3][:, x3] - sat[y0][:, x3] - sat[y3][:, x0] + sat[y0][:, x0]
            A = ((y3 - y0)[:, None] * (x3 - x0)[None, :])[:, :, None]
            res[y1:y2 + 1, x1:x2 + 1] = (S + A // 2) // A
        out.append(torch.from_numpy(res).to(image.device))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from dan_amd.utility import draw_toolbox, redact
    dev = torch.device("cuda:0")
    images, sets, num = _inputs(dev)
    buffers = redact.apply(images, sets["small"], num)
    copies = [torch.empty_like(im) for im in images]
    scratch = [im.clone() for im in images]                       # draw works in place: on copies, so that the inputs stay what they are
    classes = [torch.ones((ROWS,), dtype=torch.int32, device=dev) for _ in images]

    def redact_arm(dets, **kw):
        return lambda: redact.apply(images, dets, num, out=buffers, **kw)

    def copy_arm():
        for c, im in zip(copies, images):
            c.copy_(im)

    def draw_arm(dets):
        return lambda: draw_toolbox.bboxes_draw_on_img_list(scratch, classes, [dets[b, :, 4] for b in range(len(images))],
                                                            [dets[b, :, :4] for b in range(len(images))], thickness=2)

    arms = {"copy": copy_arm}
    for which in ("small", "large"):
        arms["draw/" + which] = draw_arm(sets[which])
        for mode in ("blur", "mosaic", "fill"):
            for shape in ("rect", "ellipse"):
                arms["redact/%s/%s/%s" % (which, mode, shape)] = redact_arm(sets[which], mode=mode, shape=shape)
    for e, strength in ((4, 4 / 500.0), (32, 32 / 500.0), (255, 1.0)):
        arms["blur/fixed/e=%d" % e] = redact_arm(sets["fixed"], strength=strength)

    want = host_blur(images, sets["large"], num)
    got, count = redact.apply(images, sets["large"], num)
    # the host path paints rows in ascending order from the original, as the rule does
    same = all(torch.equal(a, b) for a, b in zip(want, got))

    def sample(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.launches):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.launches * 1e3

    for fn in arms.values():
        sample(fn)
    times = {k: [] for k in arms}
    names = list(arms)
    for r in range(args.repeats):
        for k in range(len(names)):
            name = names[(k + r) % len(names)]
            times[name].append(sample(arms[name]))
    host_times = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_blur(images, sets["large"], num)
        torch.cuda.synchronize()
        host_times.append((time.perf_counter() - t0) * 1e6)
    times["host/large/blur/rect"] = host_times
    result = {"device": torch.cuda.get_device_name(0), "images": len(HEIGHTS), "width": W, "heights": list(HEIGHTS), "rows_per_image": ROWS,
              "bytes_per_call": 2 * sum(3 * W * h for h in HEIGHTS), "repeats": args.repeats, "launches": args.launches,
              "redacted_rows_large": int(count.item()), "device_equals_host_path_large_blur": bool(same)}
    for name, t in times.items():
        result[name + "_us"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
        print("%-32s median %10.1f us (min %.1f, max %.1f)" % (name, statistics.median(t), min(t), max(t)))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
