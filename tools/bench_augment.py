"""Device pass of the training input pipeline: the per-image loop (augment_image x 16 + torch.stack) against the batched call
(augment_batch -> danhip_augment_preprocess_batch) on the same decoded group, from uint8 device images to the network input.

    python tools/bench_augment.py [--repeats 20] [--iters 50] [--warmup 10] [--out-size 640] [--seed 0] [--contrast 1]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_augment.py --repeats 1 --iters 5     (kernel times, in a run of its own)

The group: 16 images at WIDER-like sizes, a seeded mix around 1024 x 768 with two outliers (300 x 400 and 2000 x 1400), each with the full
colour chain of preprocess_for_train (one of the four orderings; --contrast 0 drops the contrast op: the one-launch form), a window of
0.3 .. 1 x the shorter side and a flip.  The two paths run in alternating repeats; a repeat is --iters passes between two device
synchronisations.  Prints one JSON line: per-batch time of each path (median and spread over the repeats, device events), host time per
batch (the enqueue alone, before the synchronise), and the batched image kernel's algorithmic bytes (every source pixel inside a window read
once, every output pixel written once at 16 bytes)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def make_group(seed, dev, contrast):
    from dan_amd.preprocessing import dan_preprocessing as P
    rng = np.random.RandomState(seed)
    sizes = [(int(768 + rng.randint(-160, 161)), int(1024 + rng.randint(-200, 201))) for _ in range(14)]
    sizes = [s if rng.rand() < 0.7 else (s[1], s[0]) for s in sizes]
    sizes.insert(3, (300, 400))
    sizes.insert(11, (1400, 2000))
    images, params, src_bytes = [], [], 0
    draws = P.Draws(seed)
    for h, w in sizes:
        images.append(torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)).to(dev))
        ops = P.distort_color(draws.randint(0, 4), draws)
        if not contrast:
            ops = [o for o in ops if o[0] != "contrast"]
        side = int(draws.uniform(0.3, 1.) * min(h, w))
        y, x = draws.randint(0, h - side + 1), draws.randint(0, w - side + 1)
        params.append((ops, (y, x, side, side), bool(draws.uniform(0., 1.) < 0.5)))
        src_bytes += side * side * 3                                              # the window lies inside the image here
    return images, params, sizes, src_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out-size", type=int, default=640)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--contrast", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment: no GPU (there is no CPU fallback to time)")
    from dan_amd.preprocessing import dan_preprocessing as P
    dev = torch.device("cuda", 0)
    images, params, sizes, src_bytes = make_group(a.seed, dev, a.contrast)
    out_shape = (a.out_size, a.out_size)

    def per_image():
        return torch.stack([P.augment_image(im, ops, win, flip, out_shape) for im, (ops, win, flip) in zip(images, params)])

    def batched():
        return P.augment_batch(images, params, out_shape)

    for _ in range(a.warmup):
        ref, got = per_image(), batched()
    diff = (ref.float() - got.float()).abs()
    equal = {"share_of_differing_values": float((diff > 0).float().mean()), "largest_difference": float(diff.max())}

    def timed(fn):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        for _ in range(a.iters):
            fn()
        end.record()
        host = time.perf_counter() - t0                                            # the enqueue alone
        torch.cuda.synchronize()
        return start.elapsed_time(end) / a.iters, host * 1e3 / a.iters

    res = {"per_image": [], "batched": []}
    for _ in range(a.repeats):                                                     # alternating
        res["per_image"].append(timed(per_image))
        res["batched"].append(timed(batched))

    def stats(rows, i):
        v = np.asarray([r[i] for r in rows])
        return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "std_ms": float(v.std())}

    out_bytes = len(images) * a.out_size * a.out_size * 16
    print(json.dumps({"bench": "augment", "images": len(images), "sizes": sizes, "out": list(out_shape), "contrast": a.contrast, "repeats": a.repeats,
                      "iters": a.iters, "per_image_ms": stats(res["per_image"], 0), "batched_ms": stats(res["batched"], 0),
                      "per_image_host_ms": stats(res["per_image"], 1), "batched_host_ms": stats(res["batched"], 1),
                      "batched_vs_per_image": equal, "image_kernel_algorithmic_bytes": {"read": src_bytes, "written": out_bytes},
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()
