"""What the LFPN's transposed convolution costs: the PyramidBox training step (640 x 640, batch 16, the build's 16-bit type) with
lfpn_upsample "bilinear" and "transposed", alternating in one process on one device, and the three new kernels alone at the LFPN's shapes.

    python tools/bench_lfpn_upsample.py [--batch 16] [--size 640] [--steps 10] [--warmup 3] [--rounds 5] [--out profiles/r20/lfpn_transposed.md]

Two trainers are built from one seed; a round times `steps` eager steps of one, then of the other, and the next round takes them in the
other order (device events around each window, one synchronise at its end).  Reported: the median over the rounds of ms / step with the
spread (min .. max), and the ratio of the medians.  The kernels: forward, data gradient and weight + bias gradient at 20^2 -> 40^2 x 512,
40^2 -> 80^2 x 512 and 80^2 -> 160^2 x 256 channels, each timed as `reps` back-to-back launches after a warm-up, median of `rounds` windows,
with the rate in TFLOP/s of its 2 x 16 Cin Cout Hi Wi N operations.  No device: the tool fails (it does not fall back)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

LEVELS = ((20, 512), (40, 512), (80, 256))       # (Hi = Wi, channels) of lfpn/fpn_2, fpn_1, fpn_0 at 640 x 640


def _window(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def _stat(xs):
    return statistics.median(xs), min(xs), max(xs)


def bench_kernels(B, dev, reps, rounds):
    from dan_amd import _lib
    L = _lib.lib()
    rows = []
    for hi, c in LEVELS:
        dims = (B, hi, hi, 2 * hi, 2 * hi, c, c)
        g = torch.Generator().manual_seed(hi)
        x = torch.randn((B, hi, hi, c), generator=g).to(_lib.ACT_DTYPE).to(dev)
        dout = torch.randn((B, 2 * hi, 2 * hi, c), generator=g).to(_lib.ACT_DTYPE).to(dev)
        lateral = torch.randn((B, 2 * hi, 2 * hi, c), generator=g).to(_lib.ACT_DTYPE).to(dev)
        w = (0.02 * torch.randn((4, 4, c, c), generator=g)).to(dev)
        b = torch.zeros(c, device=dev)
        wf = torch.empty((4, 4, c, c), dtype=_lib.ACT_DTYPE, device=dev)
        wb = torch.empty_like(wf)
        _lib.call("danhip_conv_transpose4x4s2_pack_weight", _lib.ptr(w), _lib.ptr(wf), _lib.ptr(wb), c, c, _lib.stream())
        out, dx = torch.empty_like(dout), torch.empty_like(x)
        dw, db = torch.zeros_like(w), torch.zeros_like(b)
        nws = int(L.danhip_conv_transpose4x4s2_wgrad_workspace_bytes(*dims))
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        st = _lib.stream()
        calls = {
            "forward": lambda: _lib.call("danhip_conv_transpose4x4s2_add_fwd", _lib.ptr(x), _lib.ptr(wf), _lib.ptr(b), _lib.ptr(lateral), _lib.ptr(out), *dims, st),
            "data gradient": lambda: _lib.call("danhip_conv_transpose4x4s2_dgrad", _lib.ptr(dout), _lib.ptr(wb), _lib.ptr(dx), *dims, 0, st),
            "weight gradient": lambda: _lib.call("danhip_conv_transpose4x4s2_wgrad", _lib.ptr(x), _lib.ptr(dout), _lib.ptr(dw), _lib.ptr(db), *dims, _lib.ptr(ws), nws, st),
        }
        flop = 2.0 * 16 * c * c * hi * hi * B
        for name, fn in calls.items():
            _window(fn, 3)
            med, lo, hi_ms = _stat([_window(fn, reps) for _ in range(rounds)])
            rows.append((name, "%dx%d -> %dx%d x %d" % (hi, hi, 2 * hi, 2 * hi, c), med, lo, hi_ms, flop / med * 1e-9,
                         int(L.danhip_conv_transpose4x4s2_wgrad_slabs(*dims)) if name == "weight gradient" else None))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lfpn_upsample: no GPU")
    from dan_amd import _lib, synthetic
    from dan_amd.train_pb import PBAnchorTargets, PBModel, PBTrainer
    dev = torch.device("cuda:0")
    B, S = a.batch, a.size
    imgs = synthetic.make_images(B, S, S, dev, seed=17)
    targets = PBAnchorTargets(S, S, dev).encode_batch(synthetic.make_gt_boxes(B, S, S, seed=5, max_faces=6))
    modes = ("bilinear", "transposed")
    trainers = {m: PBTrainer(PBModel(device=dev, seed=11, lfpn_upsample=m)) for m in modes}
    for tr in trainers.values():
        for _ in range(a.warmup):
            tr.train_step(imgs, targets)
    torch.cuda.synchronize()
    times = {m: [] for m in modes}
    for r in range(a.rounds):
        for m in (modes if r % 2 == 0 else modes[::-1]):
            times[m].append(_window(lambda: trainers[m].train_step(imgs, targets), a.steps))
    for tr in trainers.values():
        tr.close()
    stats = {m: _stat(times[m]) for m in modes}
    ratio = stats["transposed"][0] / stats["bilinear"][0]
    lines = ["PyramidBox training step, %d x %d, batch %d, %s, %d rounds of %d steps, alternating order (ms / step: median, min .. max)" %
             (S, S, B, _lib.ACT_NAME, a.rounds, a.steps)]
    for m in modes:
        lines.append("  %-10s %8.3f  (%.3f .. %.3f)" % ((m,) + stats[m]))
    lines.append("  transposed / bilinear = %.4f   (FLOP share 1.014; acceptance <= 1.05)" % ratio)
    rows = bench_kernels(B, dev, a.reps, a.rounds)
    lines.append("")
    lines.append("The new kernels alone, batch %d (ms: median, min .. max of %d windows of %d launches; TFLOP/s of 2 x 16 Cin Cout Hi Wi N)" % (B, a.rounds, a.reps))
    for name, shape, med, lo, hi, tf, slabs in rows:
        lines.append("  %-16s %-28s %8.3f  (%.3f .. %.3f)  %7.1f TFLOP/s%s" % (name, shape, med, lo, hi, tf, "" if slabs is None else "  %d slabs" % slabs))
    per = {n: sum(r[2] for r in rows if r[0] == n) for n in ("forward", "data gradient", "weight gradient")}
    lines.append("  sum over the three levels: forward %.3f, data gradient %.3f, weight gradient %.3f ms; step difference %.3f ms" %
                 (per["forward"], per["data gradient"], per["weight gradient"], stats["transposed"][0] - stats["bilinear"][0]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
