"""Test-time pipeline on images of DIFFERENT sizes: eval_dan.detect_image_list against a loop of detect_image over the same images, in the same
process, on the S3FD graph with the 16-bit path.

    python tools/bench_eval_ragged.py [--repeats 7] [--out FILE.json]

8 random images, 1024 wide, heights 683, 768, 1366, 576, 1024, 731, 819, 1536; pyramid False and True.  Per configuration: one warm-up of each
path (anchor caches, allocator), then `repeats` timed runs of each in the order list -> loop and again in the order loop -> list; a run is
bracketed by torch.cuda.synchronize(), the figure is the median, the spread (min .. max) is printed with it.  The loop's result is read per
image as detect_image returns it (its bbox_vote reads the count back); the list form's result stays on the device.  One JSON line at the end."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEIGHTS = (683, 768, 1366, 576, 1024, 731, 819, 1536)
WIDTH = 1024


def _timed(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from dan_amd import eval_dan as P
    from dan_amd import train_sfd
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(0)
    imgs = [torch.from_numpy(rng.randint(0, 256, (h, WIDTH, 3)).astype(np.uint8)).to(dev) for h in HEIGHTS]
    net = P.Detector(train_sfd.SFDModel(device=dev), lambda h, w, d: train_sfd.AnchorConfig(h, w, d))
    result = {"device": torch.cuda.get_device_name(0), "images": len(imgs), "width": WIDTH, "heights": list(HEIGHTS), "repeats": args.repeats, "ms": {}}
    for pyramid in (False, True):
        as_list = lambda: P.detect_image_list(net, imgs, pyramid=pyramid)
        as_loop = lambda: [P.detect_image(net, im, pyramid=pyramid) for im in imgs]
        out, num = as_list()
        refs = as_loop()
        same = all(int(num[b]) == refs[b].shape[0] and torch.equal(out[b, :refs[b].shape[0]], refs[b]) for b in range(len(imgs)))
        times = {"list": [], "loop": []}
        for order in (("list", "loop"), ("loop", "list")):
            for name in order:
                times[name] += _timed(as_list if name == "list" else as_loop, args.repeats)
        entry = {"bitwise_equal": bool(same), "passes": sum(len(P.scale_passes(h, WIDTH, pyramid)) for h in HEIGHTS)}
        for name, t in times.items():
            entry[name] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
            print("pyramid=%s %s: median %.2f ms for %d images (min %.2f, max %.2f)" % (pyramid, name, entry[name]["median"], len(imgs), min(t), max(t)))
        entry["loop_over_list"] = entry["loop"]["median"] / entry["list"]["median"]
        result["ms"]["pyramid" if pyramid else "no_pyramid"] = entry
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
