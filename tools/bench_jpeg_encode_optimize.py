"""JpegEncoder(optimize=True) measured (no threshold is set; profiles/r21/jpeg_encode_optimize.md keeps the results).

    python tools/bench_jpeg_encode_optimize.py [--repeats 7] [--out FILE.json]
    python tools/bench_jpeg_encode_optimize.py --default_only [--package_root DIR] [--repeats 7] [--out FILE.json]

8 images of 1024 x 768 (the smooth content of tools/bench_jpeg_encode.py, so that the files have a photograph's size), quality 75, 4:2:0,
encoded from the same device tensors.  Four arms - host and device entropy stage, each without and with optimize - alternate inside every
repeat in a rotating order, 2 x `repeats` timed runs per arm, each bracketed by torch.cuda.synchronize(); the figure is the median with
its min .. max.  The files of the two optimised arms are compared with each other and with Pillow's save(optimize=True), the sizes with
and without optimize are printed.

--default_only times the two arms without optimize alone and passes no `optimize` keyword, so that it also runs on a tree from before the
keyword existed: --package_root DIR imports dan_amd from DIR (a checkout of another commit with its own built library).  Runs of this
tree and of the other in separate processes, taken in turn, are the comparison of the default path across the two commits."""
import argparse
import io
import json
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from bench_jpeg_encode import _smooth  # noqa: E402

H, W, N = 768, 1024, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--default_only", action="store_true")
    ap.add_argument("--package_root", default=os.path.dirname(HERE))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package_root))
    import torch
    from dan_amd.dataset.jpeg import JpegEncoder
    dev = torch.device("cuda:0")
    arrays = [_smooth(H, W, k) for k in range(N)]
    imgs = [torch.from_numpy(a).to(dev) for a in arrays]
    encoders = {"host": JpegEncoder(quality=75, threads=8), "device": JpegEncoder(quality=75, threads=8, entropy="device")}
    if not args.default_only:
        encoders["host_optimize"] = JpegEncoder(quality=75, threads=8, optimize=True)
        encoders["device_optimize"] = JpegEncoder(quality=75, threads=8, entropy="device", optimize=True)
    first = {name: e.encode_batch(imgs) for name, e in encoders.items()}          # also the warm-up
    result = {"device": torch.cuda.get_device_name(0), "package_root": os.path.abspath(args.package_root), "repeats": args.repeats,
              "images": N, "size": [H, W], "bytes_equal_default": first["host"] == first["device"],
              "file_bytes": sum(len(d) for d in first["host"])}
    if not args.default_only:
        from PIL import Image
        want = []
        for a in arrays:
            b = io.BytesIO()
            Image.fromarray(a).save(b, "JPEG", quality=75, optimize=True)
            want.append(b.getvalue())
        result["bytes_equal_optimize"] = first["host_optimize"] == first["device_optimize"] == want
        result["file_bytes_optimize"] = sum(len(d) for d in want)
        result["file_bytes_each"] = [[len(p), len(o)] for p, o in zip(first["host"], want)]
        result["entropy_retry"] = encoders["device_optimize"].stats["entropy_retry"]
    names = list(encoders)
    times = {name: [] for name in names}
    for r in range(2 * args.repeats):
        for k in range(len(names)):
            name = names[(k + r) % len(names)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            encoders[name].encode_batch(imgs)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name in names:
        t = times[name]
        result[name] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
        print("%s: median %.3f ms for %d images (min %.3f, max %.3f)" % (name, result[name]["median"], N, min(t), max(t)))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
