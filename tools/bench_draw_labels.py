"""The draw launch with and without the score labels, measured (no threshold; profiles/r20/draw_labels.md keeps the result).

    python tools/bench_draw_labels.py [--repeats 9] [--launches 20] [--out FILE.json]

8 images of 1024 x 768 with 200 boxes each (faces of 12 .. 200 pixels, scores in [0.2, 1], every box drawn) in ONE launch:
danhip_draw_boxes_u8 against danhip_draw_boxes_labels_u8 on the same item table and the same device tensors.  A timed window is `launches`
back-to-back launches between two device events; the two arms alternate inside every repeat in a rotating order; the figure is the median
per launch, the spread (min .. max) is printed with it.  For scale, JpegEncoder.encode_batch of the same 8 images - what follows the draw
in the evaluation command - is timed with a host clock around a synchronised call.  The labelled picture is compared with draw_reference
on one image first."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_IMAGES, H, W, N_BOXES = 8, 768, 1024, 200


def _inputs(dev):
    rng = np.random.RandomState(20)
    images = [torch.from_numpy(rng.randint(0, 200, (H, W, 3)).astype(np.uint8)).to(dev) for _ in range(N_IMAGES)]
    side = np.exp(rng.rand(N_IMAGES * N_BOXES, 1) * np.log(200 / 12.0)) * 12
    xy = rng.rand(N_IMAGES * N_BOXES, 2) * [W - 12, H - 12]
    boxes = np.concatenate([xy, xy + side * [0.8, 1.0]], 1).astype(np.float32)
    scores = (0.2 + 0.8 * rng.rand(N_IMAGES * N_BOXES)).astype(np.float32)
    return images, boxes, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from dan_amd import _lib
    from dan_amd.dataset.jpeg import JpegEncoder
    from dan_amd.utility import draw_toolbox as D
    dev = torch.device("cuda:0")
    images, boxes_np, scores_np = _inputs(dev)
    first = D.bboxes_draw_on_img(images[0], torch.ones(N_BOXES, dtype=torch.int32), torch.from_numpy(scores_np[:N_BOXES]),
                                 torch.from_numpy(boxes_np[:N_BOXES]), inplace=False, labels=True).cpu().numpy()
    exact = bool(np.array_equal(first, D.draw_reference(images[0].cpu().numpy(), [1] * N_BOXES, boxes_np[:N_BOXES], 2, scores=scores_np[:N_BOXES])))

    boxes, scores = torch.from_numpy(boxes_np).to(dev), torch.from_numpy(scores_np).to(dev)
    classes = torch.ones(N_IMAGES * N_BOXES, dtype=torch.int32, device=dev)
    items = (_lib.DrawItem * N_IMAGES)()
    for i, im in enumerate(images):
        items[i].image, items[i].width, items[i].height = im.data_ptr(), W, H
        items[i].first_box, items[i].num_boxes, items[i].groups, items[i].reserved = i * N_BOXES, N_BOXES, (W * H + 255) // 256, 0
    table = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(dev)
    n = N_IMAGES * N_BOXES
    arms = {
        "rectangles": lambda: _lib.call("danhip_draw_boxes_u8", items, _lib.ptr(table), N_IMAGES, _lib.ptr(boxes), _lib.ptr(classes), n, 2, _lib.stream()),
        "labels": lambda: _lib.call("danhip_draw_boxes_labels_u8", items, _lib.ptr(table), N_IMAGES, _lib.ptr(boxes), _lib.ptr(classes),
                                    _lib.ptr(scores), n, 2, _lib.stream()),
    }

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.launches):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.launches * 1e3                          # microseconds per launch

    for fn in arms.values():                                                    # warm-up: code objects, clocks
        window(fn)
    times = {k: [] for k in arms}
    names = list(arms)
    for r in range(args.repeats):
        for k in range(len(names)):
            name = names[(k + r) % len(names)]
            times[name].append(window(arms[name]))

    enc = JpegEncoder(quality=75)
    enc.encode_batch(images)
    encode = []
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.encode_batch(images)
        torch.cuda.synchronize()
        encode.append((time.perf_counter() - t0) * 1e6)

    result = {"device": torch.cuda.get_device_name(0), "images": N_IMAGES, "size": [H, W], "boxes_per_image": N_BOXES, "launches_per_window": args.launches,
              "repeats": args.repeats, "labelled_picture_equals_reference": exact}
    for name, t in list(times.items()) + [("encode_batch", encode)]:
        result[name + "_us"] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
        print("%s: median %.1f us (min %.1f, max %.1f)" % (name, statistics.median(t), min(t), max(t)))
    result["labels_over_rectangles"] = result["labels_us"]["median"] / result["rectangles_us"]["median"]
    result["labels_share_of_encode"] = result["labels_us"]["median"] / result["encode_batch_us"]["median"]
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
