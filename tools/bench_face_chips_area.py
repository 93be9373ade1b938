"""Face chips measured by filter and padding (no threshold is set; profiles/r25/face_chips_area.md keeps the result).

    python tools/bench_face_chips_area.py [--repeats 9] [--size 112] [--out FILE.json]

Two sets on the same 8 images 1024 wide (tools/bench_face_chips.py's): `mixed`, its 40 detections per image with sides 16 .. 400 px, and
`large`, 40 detections per image 300 .. 600 px wide, where the area form reads (n / S + 1)^2 source pixels per output pixel.  Four arms
per set: filter linear / area x pad off / on, each utility.face_chips.extract into buffers made once (linear without pad is the old entry
point, the other three danhip_face_chips_u8_ex).  A timed sample is ONE call between two torch.cuda.synchronize() on a host clock; the
arms alternate inside every repeat in a rotating order; the figure is the median, the spread (min .. max) is printed with it.  The device
time of the launches alone (device events around `launches` back-to-back calls) is reported beside it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench_face_chips as base  # noqa: E402

ARMS = [("linear", False), ("linear", True), ("area", False), ("area", True)]


def _large(dev):
    rng = np.random.RandomState(25)
    dets = np.zeros((len(base.HEIGHTS), base.ROWS, 5), np.float32)
    for i, h in enumerate(base.HEIGHTS):
        wide = 300 + 300 * rng.rand(base.ROWS)
        x1, y1 = rng.rand(base.ROWS) * (base.W - 200) - 100, rng.rand(base.ROWS) * (h - 200) - 100      # some leave the image
        dets[i] = np.stack([x1, y1, x1 + wide, y1 + wide / 0.8, 0.2 + 0.8 * rng.rand(base.ROWS)], 1)
    return torch.from_numpy(dets).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from dan_amd.utility import face_chips
    dev = torch.device("cuda:0")
    images, mixed, num = base._inputs(dev)
    S = args.size
    result = {"device": torch.cuda.get_device_name(0), "images": len(base.HEIGHTS), "width": base.W, "heights": list(base.HEIGHTS),
              "rows_per_image": base.ROWS, "size": S, "repeats": args.repeats, "sets": {}}

    def sample(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    for set_name, dets in (("mixed", mixed), ("large", _large(dev))):
        arms, chips = {}, {}
        for filt, pad in ARMS:
            buffers = tuple(face_chips.extract(images, dets, num, size=S, filter=filt, pad=pad))      # made once, reused by every timed call
            name = "%s%s" % (filt, "+pad" if pad else "")
            arms[name] = (lambda f=filt, p=pad, b=buffers: face_chips.extract(images, dets, num, size=S, filter=f, pad=p, out=b))
            chips[name] = int(buffers[2].item())
        for fn in arms.values():
            sample(fn)
        times, names = {k: [] for k in arms}, list(arms)
        for r in range(args.repeats):
            for k in range(len(names)):
                name = names[(k + r) % len(names)]
                times[name].append(sample(arms[name]))
        out = result["sets"][set_name] = {}
        for name in names:
            device_only = []
            for _ in range(args.repeats):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.launches):
                    arms[name]()
                b.record()
                b.synchronize()
                device_only.append(a.elapsed_time(b) / args.launches * 1e3)
            out[name] = {"chips": chips[name]}
            for key, t in (("call_us", times[name]), ("back_to_back_us", device_only)):
                out[name][key] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
                print("%s %s %s: median %.1f us (min %.1f, max %.1f), %d chips" % (set_name, name, key, statistics.median(t), min(t), max(t), chips[name]))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
