"""Wall time of saving and restoring the S3FD trainer's checkpoint, and the rate of the CRC-32C batch kernel.

    python tools/bench_checkpoint.py [--repeats 9] [--size 640] [--batch 16] [--dir DIR] [--python-slice-mb 2]

The trainer is bench.py's (S3FD, one step taken so that weights and momenta are not their initial patterns).  In every repeat the
variants run one after the other, and the order is reversed in every other repeat:
    save_unchecked   Trainer.save(checksums=False)      - the code of the parent commit, unchanged here (one .cpu() per tensor, no CRC)
    save_host        Trainer.save(checksums=True)       - one .cpu() per tensor, danhip_crc32c_host per tensor
    save_device      Trainer.save(checksums="device")   - shard packed and checksummed on the GPU, one copy down
    restore          Trainer.restore(verify=False)      - the parent's restore
    restore_verify   Trainer.restore(verify=True)       - shard uploaded once, one batch call, variables filled from the device image
A timing is a host clock around a call that ends synchronised (the save has written its files; the restore is followed by a device
synchronise).  save_python_scaled is NOT run: the parent's checksums=True used the pure-Python loop, which is timed on a --python-slice-mb
slice of the shard and scaled to the shard's size, then added to save_unchecked's median.
The kernel rate: device events around danhip_crc32c_batch over the packed shard (all tensors in one call), both walk forms, beside a
device-to-device copy of the same bytes (tools/calibrate_peaks.py's copy stream at this size, counted as read + write).
Prints a table and one JSON line."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def spread(xs):
    return {"median_ms": round(statistics.median(xs) * 1e3, 2), "min_ms": round(min(xs) * 1e3, 2), "max_ms": round(max(xs) * 1e3, 2), "n": len(xs)}


def events_ms(f, iters, warm=3):
    for _ in range(warm):
        f()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dir", default=None, help="where the checkpoints are written (default: a temporary directory, removed afterwards)")
    ap.add_argument("--python-slice-mb", type=float, default=2.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_checkpoint: no GPU (nothing here can be timed without one)")
    from dan_amd import _lib, synthetic
    from dan_amd.train_sfd import AnchorConfig, SFDModel, SFDTrainer
    from dan_amd.utility import checkpoint as C
    dev = torch.device("cuda", 0)
    tr = SFDTrainer(SFDModel(device=dev, seed=1))
    imgs = synthetic.make_images(a.batch, a.size, a.size, dev, seed=3)
    loc_t, cls_t, _ = AnchorConfig(a.size, a.size, dev).encode_batch(synthetic.make_gt_boxes(a.batch, a.size, a.size, seed=2, max_faces=4))
    tr.train_step(imgs, loc_t, cls_t)
    torch.cuda.synchronize()
    root = a.dir or tempfile.mkdtemp(prefix="danhip_ckpt_")
    os.makedirs(root, exist_ok=True)
    prefix = lambda name: os.path.join(root, name, "model.ckpt-1")

    def save(kind, checksums):
        def run():
            t0 = time.perf_counter()
            tr.save(prefix(kind), "sfd", checksums=checksums)
            return time.perf_counter() - t0
        return run

    def restore(verify):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.restore(prefix("save_device"), "sfd", verify=verify)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        return run

    variants = [("save_unchecked", save("save_unchecked", False)), ("save_host", save("save_host", True)),
                ("save_device", save("save_device", "device")), ("restore", restore(False)), ("restore_verify", restore(True))]
    for _, f in variants:                                                  # warm-up: pinned buffers, code objects, page cache
        f()
    times = {n: [] for n, _ in variants}
    for r in range(a.repeats):
        for n, f in (variants if r % 2 == 0 else variants[::-1]):
            times[n].append(f())
    data_path = prefix("save_device") + ".data-00000-of-00001"
    shard_bytes = os.path.getsize(data_path)
    same = all(open(prefix(k) + s, "rb").read() == open(prefix("save_device") + s, "rb").read()
               for k in ("save_host",) for s in (".index", ".data-00000-of-00001"))
    out = {"what": "S3FD trainer checkpoint: weights, Momentum slots, global_step", "shard_bytes": shard_bytes,
           "tensors": len(C.CheckpointReader(prefix("save_device")).entries), "device_files_equal_host_files": same,
           "times": {n: spread(v) for n, v in times.items()}}
    # the parent's checksums=True: the Python loop on a slice, scaled
    n_slice = int(a.python_slice_mb * (1 << 20))
    blob = open(data_path, "rb").read(n_slice)
    t0 = time.perf_counter()
    C._crc32c_py(blob)
    per_byte = (time.perf_counter() - t0) / len(blob)
    out["save_python_scaled"] = {"slice_bytes": len(blob), "python_MBps": round(1e-6 / per_byte, 2),
                                 "scaled_ms": round((per_byte * shard_bytes + statistics.median(times["save_unchecked"])) * 1e3, 0),
                                 "note": "NOT run in full: the Python loop timed on the slice, scaled to the shard, plus save_unchecked's median"}
    # host entry rate
    whole = open(data_path, "rb").read()
    t0 = time.perf_counter()
    C.crc32c(whole)
    out["host_entry_GBps"] = round(len(whole) / (time.perf_counter() - t0) / 1e9, 2)
    # kernel rate on the packed shard, both forms, beside a copy of the same bytes
    io = tr.checkpoint_io
    reader = C.CheckpointReader(prefix("save_device"))
    image, _, nbytes = io.upload(data_path)
    ranges = [(e["offset"], e["size"]) for e in reader.entries.values()]
    L = _lib.lib()
    kern = {}
    for form, name in ((0, "table_free"), (1, "lds_table")):
        L.danhip_set_option(b"crc_table", form)
        ts = events_ms(lambda: io.crc_launch(image, ranges), 20)
        kern[name] = dict(spread(ts), GBps=round(nbytes / statistics.median(ts) / 1e9, 1))
    L.danhip_set_option(b"crc_table", 1)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ts = events_ms(lambda: dst.copy_(image[:nbytes]), 20)
    out["crc_batch_call"] = kern
    out["device_copy_same_bytes"] = dict(spread(ts), GBps_read_plus_write=round(2 * nbytes / statistics.median(ts) / 1e9, 1))
    host = io.host(nbytes)
    ts = events_ms(lambda: host[:nbytes].copy_(image[:nbytes], non_blocking=True), 10)
    out["device_to_pinned_host_copy"] = dict(spread(ts), GBps=round(nbytes / statistics.median(ts) / 1e9, 1))
    tr.close()
    if not a.dir:
        shutil.rmtree(root, ignore_errors=True)
    for n, v in out["times"].items():
        print("%-16s median %9.2f ms   (min %9.2f, max %9.2f, n=%d)" % (n, v["median_ms"], v["min_ms"], v["max_ms"], v["n"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
