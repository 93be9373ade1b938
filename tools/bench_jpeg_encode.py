"""The JPEG encoder and the evaluation command, measured (no threshold is set on either; profiles/r17/eval_driver.md keeps the results).

    python tools/bench_jpeg_encode.py [--repeats 7] [--workdir DIR] [--out FILE.json] [--encode_only]

1. Encode of 8 decoded 1024-wide images - the ragged set of tools/bench_eval_ragged.py, smooth content so that the files have a photograph's
   size - from the SAME device tensors: JpegEncoder.encode_batch (device pixel stage, one download of the coefficients, host Huffman threads)
   against JpegEncoder(entropy="device") (the Huffman stage on the device too: sizes, status words and the files come back, no
   coefficient) and against Pillow on the host (one download per image, Image.save at the same quality).  2 x `repeats` timed runs of
   each, the three alternating inside every repeat in a rotating order; a run is bracketed by torch.cuda.synchronize(); the figure is the
   median, the spread (min .. max) and the bytes each arm downloads are printed with it.  The bytes of all three are compared.
   profiles/r18/jpeg_encode_entropy.md keeps the device-entropy arm's results.
2. The command's images/s on a synthetic WIDER tree (2 events x 8 images, 640 x 480, seeded S3FD initialisers as the checkpoint):
   `dan_amd.eval_sfd.main` with --debug_dir, with --debug_dir "" and with --log_every_n_steps 1 (every image drawn and encoded), and
   eval_sfd.detect_encoded alone over the same files - alternating, median of `repeats` runs each."""
import argparse
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HEIGHTS = (683, 768, 1366, 576, 1024, 731, 819, 1536)
WIDTH = 1024


def _timed_once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _stats(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def _smooth(h, w, seed):
    rng = np.random.RandomState(seed)
    small = rng.rand(h // 32 + 2, w // 32 + 2, 3)
    big = np.kron(small, np.ones((32, 32, 1)))[:h, :w]
    yy, xx = np.mgrid[0:h, 0:w]
    return np.clip(big * 200 + 20 * np.sin(xx / 13.0)[..., None] + 20 * np.cos(yy / 17.0)[..., None] + rng.rand(h, w, 3) * 12, 0, 255).astype(np.uint8)


def bench_encode(dev, repeats):
    from PIL import Image
    from dan_amd.dataset.jpeg import JpegEncoder
    imgs = [torch.from_numpy(_smooth(h, WIDTH, k)).to(dev) for k, h in enumerate(HEIGHTS)]
    enc = JpegEncoder(quality=75, threads=8)
    enc_dev = JpegEncoder(quality=75, threads=8, entropy="device")

    def pillow():
        out = []
        for im in imgs:
            b = io.BytesIO()
            Image.fromarray(im.cpu().numpy()).save(b, "JPEG", quality=75)
            out.append(b.getvalue())
        return out
    arms = {"device": lambda: enc.encode_batch(imgs), "device_entropy": lambda: enc_dev.encode_batch(imgs), "pillow": pillow}
    first = {name: fn() for name, fn in arms.items()}            # also the warm-up of all three
    same = first["device"] == first["pillow"] == first["device_entropy"]
    downloads = {}
    for name, e in (("device", enc), ("device_entropy", enc_dev)):
        before = e.stats["download_bytes"]
        arms[name]()
        downloads[name] = e.stats["download_bytes"] - before
    downloads["pillow"] = sum(int(im.numel()) for im in imgs)
    times = {name: [] for name in arms}
    names = list(arms)
    for r in range(2 * repeats):                                 # the three arms alternate inside every repeat, the order rotates
        for k in range(len(names)):
            name = names[(k + r) % len(names)]
            times[name].append(_timed_once(arms[name]))
    entry = {"bytes_equal": bool(same), "images": len(imgs), "file_bytes": sum(len(d) for d in first["device"]), "download_bytes": downloads,
             "entropy_retry": enc_dev.stats["entropy_retry"]}
    for name in names:
        entry[name] = _stats(times[name])
        print("encode %s: median %.2f ms for %d images (min %.2f, max %.2f), %d bytes downloaded" %
              (name, entry[name]["median"], len(imgs), entry[name]["min"], entry[name]["max"], downloads[name]))
    entry["pillow_over_device"] = entry["pillow"]["median"] / entry["device"]["median"]
    entry["device_over_device_entropy"] = entry["device"]["median"] / entry["device_entropy"]["median"]
    return entry


def bench_command(dev, repeats, workdir):
    from dan_amd import eval_cli, eval_sfd
    from dan_amd.dataset.jpeg import JpegDecoder, JpegEncoder
    from dan_amd.utility import checkpoint
    events = [("0--Parade", ["0_%02d" % k for k in range(8)]), ("1--Handshaking", ["1_%02d" % k for k in range(8)])]
    enc = JpegEncoder(quality=90)
    datas = []
    for e, (event, names) in enumerate(events):
        os.makedirs(os.path.join(workdir, "WIDER_val", "images", event), exist_ok=True)
        for k, name in enumerate(names):
            data = enc.encode(_smooth(480, 640, 100 + 8 * e + k))
            datas.append(data)
            with open(os.path.join(workdir, "WIDER_val", "images", event, name + ".jpg"), "wb") as f:
                f.write(data)
    with open(os.path.join(workdir, "list.txt"), "w") as f:
        f.write("".join("%s/%s\n" % (event, n) for event, names in events for n in names))
    net = eval_cli.build_detector("sfd", dev, "act")
    os.makedirs(os.path.join(workdir, "logs"), exist_ok=True)
    checkpoint.save_checkpoint(net.model.vs, os.path.join(workdir, "logs", "model.ckpt-1"), "sfd", checksums=True)
    common = ["--data_dir", workdir, "--image_list", os.path.join(workdir, "list.txt"), "--det_dir", os.path.join(workdir, "det"),
              "--checkpoint_path", os.path.join(workdir, "logs", "model.ckpt-1")]
    dec = JpegDecoder(dev)
    runs = {
        "command_debug_every_10": lambda: eval_sfd.main(common + ["--debug_dir", os.path.join(workdir, "debug")], out=io.StringIO()),
        "command_no_debug": lambda: eval_sfd.main(common + ["--debug_dir", ""], out=io.StringIO()),
        "command_debug_every_image": lambda: eval_sfd.main(common + ["--debug_dir", os.path.join(workdir, "debug"), "--log_every_n_steps", "1"], out=io.StringIO()),
        "detect_encoded_alone": lambda: [eval_sfd.detect_encoded(net, datas[a:a + 8], dec) for a in (0, 8)],
    }
    for fn in runs.values():
        fn()                                                     # warm-up: anchor caches, allocator, code objects
    times = {k: [] for k in runs}
    for r in range(repeats):
        for name in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
            times[name].append(_timed_once(runs[name]))
    entry = {"images": len(datas), "size": [480, 640]}
    for name, t in times.items():
        entry[name] = _stats(t)
        entry[name]["images_per_s"] = len(datas) / (entry[name]["median"] * 1e-3)
        print("%s: median %.1f ms for %d images = %.1f images/s (min %.1f, max %.1f ms)" % (name, entry[name]["median"], len(datas),
                                                                                              entry[name]["images_per_s"], min(t), max(t)))
    return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--encode_only", action="store_true", help="part 1 alone")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "encode": bench_encode(dev, args.repeats)}
    if not args.encode_only:
        with tempfile.TemporaryDirectory(dir=args.workdir) as d:
            result["command"] = bench_command(dev, args.repeats, d)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
