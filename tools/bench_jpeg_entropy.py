#!/usr/bin/env python3
"""JPEG decode throughput with the Huffman stage on the device: JpegDecoder(dev, entropy="device") - its host half is one thread - against
the default decoder at 1 / 4 / 16 host threads, on the image sets and modes of tools/bench_jpeg.py at batch 16, the paths alternating inside
every round of the same run.  Per mode: end-to-end img/s (median of the rounds, min, max), host ms per image of the prepare pass, device-event
time of the Huffman launches per batch, uploaded bytes per image on both paths, the retry count, and the ratio to the default of 4 threads -
the bar the device path is measured against.  Prints one JSON object.  Per-kernel times: a rocprofv3 --kernel-trace --stats run of this
script of its own.

    python tools/bench_jpeg_entropy.py [--images 64] [--rounds 3]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_jpeg import BATCH, H, MODES, W, device_path, encode_set            # noqa: E402
from dan_amd.dataset.jpeg import JpegDecoder                                  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_entropy.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "batch": BATCH, "images_per_mode": a.images, "modes": {}}
    for m, (name, kw) in enumerate(MODES):
        datas = encode_set(a.images, kw, 1000 * m)
        decs = {"host_threads_%d" % t: JpegDecoder(dev, threads=t) for t in (1, 4, 16)}
        decs["device_entropy"] = JpegDecoder(dev, threads=1, entropy="device")
        for dec in decs.values():
            device_path(dec, datas[:BATCH])                                   # warm-up: code objects, pinned buffer, allocator
            for k in ("entropy_seconds", "device", "upload_bytes", "entropy_retry", "entropy_device"):
                dec.stats[k] = 0
        rates = {}
        for _ in range(a.rounds):                                             # alternate the paths inside every round
            for k, dec in decs.items():
                rates.setdefault(k, []).append(device_path(dec, datas))
        row = {"jpeg_bytes_per_image": int(np.mean([len(d) for d in datas]))}
        row["images_per_s"] = {k: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for k, v in rates.items()}
        row["host_ms_per_image"] = {k: round(1e3 * d.stats["entropy_seconds"] / max(d.stats["device"], 1), 4) for k, d in decs.items()}
        row["uploaded_bytes_per_image"] = {k: int(d.stats["upload_bytes"] / max(d.stats["device"], 1)) for k, d in decs.items()}
        row["retries"] = decs["device_entropy"].stats["entropy_retry"]
        row["device_over_host_threads_4"] = round(row["images_per_s"]["device_entropy"]["median"] / row["images_per_s"]["host_threads_4"]["median"], 3)
        timed = JpegDecoder(dev, threads=1, entropy="device")                  # device events around the Huffman launches, outside the rate loop
        timed.decode_batch(datas[:BATCH])
        timed.time_huffman, timed.stats["huffman_ms"] = True, None
        for _ in range(5):
            timed.decode_batch(datas[:BATCH])
        row["huffman_launches_ms_per_batch16"] = round(timed.stats["huffman_ms"] / 5, 4)
        got, want = decs["device_entropy"].decode_batch(datas[:BATCH]), decs["host_threads_4"].decode_batch(datas[:BATCH])
        row["equal_to_default_decoder"] = all(torch.equal(g, w) for g, w in zip(got, want))
        res["modes"][name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
