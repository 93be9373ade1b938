"""Times the ResNet-50 backbone and a full DAN training step on it (bf16, 640 x 640).

    python tools/bench_resnet_dan.py --section backbone --fused 1 --batch 8      one fresh process: forward + backward of get_featmaps
    python tools/bench_resnet_dan.py --section step --batch 8                    one fresh process: DANTrainer(backbone="resnet50") steps
    python tools/bench_resnet_dan.py --compare --rounds 3 --out DIR              alternating fresh processes: unfused, fused, unfused, ...

--section backbone with --fused 0 is the unfused graph (batch norm, torch add, torch ReLU: what the tree had before the fused tail kernels;
the same script section runs against an older checkout, which has no fused_tail keyword, with --fused -1).  Times are host clock around
a device synchronise, over --steps steps after --warmup; library calls per step are those dan_amd.ops issues (counted by wrapping its `call`).  One JSON line per process."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _count_calls():
    """library calls per step, by name: wraps dan_amd._lib.call (every kernel entry point goes through it)"""
    from dan_amd import _lib, ops
    counts = {}
    inner = _lib.call

    def call(name, *a):
        counts[name] = counts.get(name, 0) + 1
        return inner(name, *a)
    _lib.call = call
    ops.call = call
    return counts


def run_backbone(args):
    import torch
    from dan_amd import synthetic
    from dan_amd.net import resnet_danet, sfd_net
    from dan_amd.net.variables import VariableStore
    dev = torch.device("cuda:0")
    kw = {} if args.fused < 0 else {"fused_tail": bool(args.fused)}
    net = resnet_danet.ResNetBackbone(50, variables=VariableStore(device=dev, seed=1), **kw)
    x = sfd_net.prepare_input(synthetic.make_images(args.batch, args.size, args.size, dev, seed=3))

    def step():
        feats = net.get_featmaps(x, training=True)
        torch.autograd.backward(feats, [torch.ones_like(f) for f in feats])
        for _, p in net.vs.named():
            p.grad = None
    for _ in range(args.warmup):
        step()
    counts = _count_calls()
    step()
    launches = dict(counts)
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    bn = sum(v for k, v in launches.items() if "batchnorm" in k or "bn_act" in k or "relu_bwd" in k)
    return dict(section="backbone", fused=args.fused, batch=args.batch, size=args.size, ms_median=statistics.median(times), ms_min=min(times),
                ms_max=max(times), library_calls=sum(launches.values()), batch_norm_calls=bn, peak_gib=torch.cuda.max_memory_allocated() / 2 ** 30)


def run_step(args):
    import torch
    from dan_amd import synthetic
    from dan_amd.train_dan import DANModel, DANTrainer, dan_anchor_config, encode_batch_dan
    dev = torch.device("cuda:0")
    anchors = dan_anchor_config(args.size, args.size, dev)
    tr = DANTrainer(DANModel(device=dev, seed=4, backbone="resnet50"), anchors)
    imgs = synthetic.make_images(args.batch, args.size, args.size, dev, seed=3)
    batch = (imgs,) + tuple(encode_batch_dan(anchors, synthetic.make_gt_boxes(args.batch, args.size, args.size, seed=2)))
    for _ in range(args.warmup):
        tr.train_step(*batch)
    counts = _count_calls()
    tr.train_step(*batch)
    launches = sum(counts.values())
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        tr.train_step(*batch)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    loss = tr.loss_values()["total"]
    tr.close()
    med = statistics.median(times)
    return dict(section="step", batch=args.batch, size=args.size, ms_median=med, ms_min=min(times), ms_max=max(times), images_per_s=args.batch / med * 1e3,
                library_calls=launches, loss=loss, peak_gib=torch.cuda.max_memory_allocated() / 2 ** 30)


def compare(args):
    os.makedirs(args.out, exist_ok=True)
    rows = []
    base = [sys.executable, os.path.abspath(__file__), "--batch", str(args.batch), "--size", str(args.size), "--steps", str(args.steps), "--warmup", str(args.warmup)]
    with open(os.path.join(args.out, "resnet_dan_bench.jsonl"), "a") as log:
        for r in range(args.rounds):
            for fused in (0, 1):
                p = subprocess.run(base + ["--section", "backbone", "--fused", str(fused)], capture_output=True, text=True, timeout=args.timeout)
                if p.returncode != 0:
                    print(p.stderr[-2000:])
                    return p.returncode
                rows.append(json.loads(p.stdout.strip().splitlines()[-1]))
                log.write(json.dumps(rows[-1]) + "\n")
                log.flush()
                print(json.dumps(rows[-1]), flush=True)
        p = subprocess.run(base + ["--section", "step"], capture_output=True, text=True, timeout=args.timeout)
        if p.returncode != 0:
            print(p.stderr[-2000:])
            return p.returncode
        log.write(p.stdout.strip().splitlines()[-1] + "\n")
        print(p.stdout.strip().splitlines()[-1], flush=True)
    for fused in (0, 1):
        med = [r["ms_median"] for r in rows if r["fused"] == fused]
        print("fused=%d: medians %s  median of medians %.2f ms  spread %.2f ms" % (fused, ["%.2f" % m for m in med], statistics.median(med), max(med) - min(med)))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--section", choices=("backbone", "step"), default="backbone")
    ap.add_argument("--fused", type=int, default=1, help="1: fused_tail=True; 0: fused_tail=False; -1: a checkout without the keyword")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default="profiles/r23")
    args = ap.parse_args()
    if args.compare:
        return compare(args)
    print(json.dumps(run_backbone(args) if args.section == "backbone" else run_step(args)), flush=True)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
