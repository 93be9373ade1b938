#!/usr/bin/env python3
"""JPEG decode throughput: the host path (dataset_common.decode_image with Pillow, one image at a time, plus the upload) against
dataset.jpeg.JpegDecoder.decode_batch at 1 / 4 / 8 / 16 host threads, batch 16, on 64 seeded 1024 x 768 images per sampling mode, the two
paths alternating in the same run.  Also: host entropy ms per image, the two launches' time (device events around
danhip_jpeg_reconstruct_batch; per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script with --kernels-only),
their algorithmic bytes/s, and the box's copy rate measured the way tools/calibrate_peaks.py measures it.  Prints one JSON object.
--progressive: the same images encoded as progressive streams; JpegDecoder(progressive=True) at 1 / 4 / 8 / 16 host threads against
JpegDecoder(progressive=False) - every image through the Pillow fallback and its own upload, what a progressive record costs by default -
the arms alternating inside every round: seconds per batch of 16 (median, min, max over rounds x batches) and the host entropy stage's share.

    python tools/bench_jpeg.py [--images 64] [--rounds 3] [--kernels-only | --progressive]"""
import argparse
import ctypes
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dan_amd import _lib                                                      # noqa: E402
from dan_amd.dataset import dataset_common as DC                              # noqa: E402
from dan_amd.dataset.jpeg import JpegDecoder                                  # noqa: E402

MODES = [("420_q90", dict(subsampling=2, quality=90)), ("422_q90", dict(subsampling=1, quality=90)), ("444_q90", dict(subsampling=0, quality=90)),
         ("420_q75_optimize", dict(subsampling=2, quality=75, optimize=True))]
H, W, BATCH = 768, 1024, 16


def encode_set(n, kw, seed):
    from PIL import Image, ImageFile
    if kw.get("progressive"):
        ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 4 * H * W)               # a progressive encode needs the whole stream in one buffer
    out = []
    for i in range(n):
        r = np.random.RandomState(seed + i)
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.stack([xx * 255 // (W - 1), yy * 255 // (H - 1), ((xx + yy) * 3) % 256], 2).astype(np.float64) + r.randn(H, W, 3) * 30
        b = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(b, format="JPEG", **kw)
        out.append(b.getvalue())
    return out


def host_path(datas, dev):
    t0 = time.perf_counter()
    keep = [torch.from_numpy(DC.decode_image(d)).to(dev) for d in datas]
    torch.cuda.synchronize()
    return len(keep) / (time.perf_counter() - t0)


def device_path(dec, datas):
    t0 = time.perf_counter()
    keep = [dec.decode_batch(datas[i:i + BATCH]) for i in range(0, len(datas), BATCH)]
    torch.cuda.synchronize()
    return sum(len(k) for k in keep) / (time.perf_counter() - t0)


def launches_time(datas, dev, it=20):
    """Device events around the two launches of one batch of 16 (coefficients already on the device)."""
    L = _lib.lib()
    B = len(datas)
    info, cap = _lib.JpegInfo(), 0
    for d in datas:
        assert L.danhip_jpeg_inspect(d, len(d), ctypes.byref(info)) == 0
        cap += info.coef_count
    coef = torch.empty(cap, dtype=torch.int16).pin_memory()
    descs, status = (_lib.JpegDesc * B)(), (ctypes.c_int32 * B)()
    _lib.call("danhip_jpeg_entropy_decode_batch", (ctypes.c_char_p * B)(*datas), (ctypes.c_int64 * B)(*[len(d) for d in datas]), B, 4,
              ctypes.c_void_p(coef.data_ptr()), cap, descs, status)
    assert list(status) == [0] * B
    coef_d = coef.to(dev)
    descs_d = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    nws, nout = L.danhip_jpeg_workspace_bytes(descs, B), L.danhip_jpeg_output_bytes(descs, B)
    ws, out = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(nout, dtype=torch.uint8, device=dev)

    def run():
        _lib.call("danhip_jpeg_reconstruct_batch", _lib.ptr(coef_d), cap, descs, _lib.ptr(descs_d), B, _lib.ptr(out), nout, _lib.ptr(ws), nws, None,
                  _lib.stream())
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(it):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / it
    planes = cap                                                              # one uint8 per coefficient
    idct_bytes, rgb_bytes = 2 * cap + planes, planes + B * H * W * 3          # read coefficients + write planes; read planes + write RGB
    return {"two_launches_ms_per_batch16": round(ms, 4), "idct_bytes": idct_bytes, "rgb_bytes": rgb_bytes,
            "two_launches_GBps_algorithmic": round((idct_bytes + rgb_bytes) / ms / 1e6, 1)}


def batch_times(dec, datas):
    """seconds of every batch of 16, each timed to the end of its device work"""
    out = []
    for i in range(0, len(datas), BATCH):
        t0 = time.perf_counter()
        keep = dec.decode_batch(datas[i:i + BATCH])
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
        del keep
    return out


def progressive_mode(a, dev):
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "batch": BATCH, "images_per_mode": a.images, "rounds": a.rounds, "modes": {}}
    for m, (name, kw) in enumerate(MODES):
        datas = encode_set(a.images, dict(kw, progressive=True), 1000 * m)
        arms = {"fallback": JpegDecoder(dev, progressive=False)}
        arms.update({"threads_%d" % t: JpegDecoder(dev, threads=t, progressive=True) for t in (1, 4, 8, 16)})
        for dec in arms.values():
            batch_times(dec, datas[:BATCH])                                   # warm-up: code objects, pinned buffer, allocator
            dec.stats["entropy_seconds"] = 0.0
        times = {k: [] for k in arms}
        for _ in range(a.rounds):                                             # alternate the arms inside every round
            for k, dec in arms.items():
                times[k] += batch_times(dec, datas)
        row = {"jpeg_bytes_per_image": int(np.mean([len(d) for d in datas])), "ms_per_batch16": {}, "entropy_ms_per_batch16": {}}
        for k, v in times.items():
            row["ms_per_batch16"][k] = {"median": round(1e3 * float(np.median(v)), 2), "min": round(1e3 * min(v), 2), "max": round(1e3 * max(v), 2), "n": len(v)}
            if k != "fallback":
                row["entropy_ms_per_batch16"][k] = round(1e3 * arms[k].stats["entropy_seconds"] / len(v), 2)
        row["fallback_over_threads_4"] = round(row["ms_per_batch16"]["fallback"]["median"] / row["ms_per_batch16"]["threads_4"]["median"], 2)
        row["fallbacks_with_progressive_on"] = sum(sum(d.stats["fallback"].values()) for k, d in arms.items() if k != "fallback")
        row["launches_per_batch_threads_4"] = arms["threads_4"].stats["launches"] / (len(times["threads_4"]) + 1)
        got = arms["threads_4"].decode_batch(datas[:BATCH])
        row["equal_to_pillow"] = all(torch.equal(g.cpu(), torch.from_numpy(DC.decode_image(d))) for g, d in zip(got, datas[:BATCH]))
        res["modes"][name] = row
    print(json.dumps(res))


def copy_rate(dev):
    n = 16 * 640 * 640 * 64                                                   # as tools/calibrate_peaks.py: 839 MB of bf16, read + write
    x = torch.zeros(n, device=dev, dtype=torch.bfloat16)
    y = torch.empty_like(x)
    for _ in range(3):
        y.copy_(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        y.copy_(x)
    e1.record()
    torch.cuda.synchronize()
    return round(2 * n * 2 / (e0.elapsed_time(e1) / 20) / 1e6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true", help="only the two launches (for a rocprofv3 --kernel-trace --stats run)")
    ap.add_argument("--progressive", action="store_true", help="progressive streams: JpegDecoder(progressive=True) against the Pillow fallback")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    if a.progressive:
        return progressive_mode(a, dev)
    res = {"device": torch.cuda.get_device_name(0), "image": [H, W], "batch": BATCH, "images_per_mode": a.images, "modes": {}}
    if not a.kernels_only:
        res["copy_GBps_read_plus_write"] = copy_rate(dev)
    for m, (name, kw) in enumerate(MODES):
        datas = encode_set(a.images, kw, 1000 * m)
        row = {"jpeg_bytes_per_image": int(np.mean([len(d) for d in datas]))}
        row.update(launches_time(datas[:BATCH], dev))
        if not a.kernels_only:
            decs = {t: JpegDecoder(dev, threads=t) for t in (1, 4, 8, 16)}
            host_path(datas[:8], dev)
            for dec in decs.values():
                device_path(dec, datas[:BATCH])                               # warm-up: code objects, pinned buffer, allocator
                dec.stats["entropy_seconds"], dec.stats["device"] = 0.0, 0
            rates = {"host": []}
            for _ in range(a.rounds):                                         # alternate the paths inside every round
                rates["host"].append(host_path(datas, dev))
                for t, dec in decs.items():
                    rates.setdefault("threads_%d" % t, []).append(device_path(dec, datas))
            row["images_per_s"] = {k: {"median": round(float(np.median(v)), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for k, v in rates.items()}
            row["entropy_ms_per_image_wall"] = {"threads_%d" % t: round(1e3 * d.stats["entropy_seconds"] / max(d.stats["device"], 1), 3) for t, d in decs.items()}
            row["fallbacks"] = sum(sum(d.stats["fallback"].values()) for d in decs.values())
            # results must not differ: the device images against the host path's, on this mode's first batch
            got = decs[4].decode_batch(datas[:BATCH])
            row["equal_to_pillow"] = all(torch.equal(g.cpu(), torch.from_numpy(DC.decode_image(d))) for g, d in zip(got, datas[:BATCH]))
        res["modes"][name] = row
    print(json.dumps(res))


if __name__ == "__main__":
    main()
