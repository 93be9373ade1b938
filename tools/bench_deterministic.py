"""What deterministic mode costs: the S3FD training step (640 x 640, bf16, batch 16) with the switch off and on, alternating in one process on
one device, plus the kernel launches the mode adds per step (a count).

    python tools/bench_deterministic.py [--model sfd|dan_deform] [--batch 16] [--size 640] [--steps 20] [--rounds 3] [--out profiles/r12/deterministic.md]

--model dan_deform times the DAN-Deform step instead (DANTrainer(DANModel(deform=True), anchors) against the same with
ops_ctx=ops.deterministic_context(): the deformable backward's ordered far-corner path, profiles/r19/deterministic_deform.md).

Two trainers are built from one seed (SFDTrainer(model) and SFDTrainer(model, deterministic=True)); each round times `steps` eager steps of
one, then of the other (device events around the window, one synchronise at its end).  Launches are counted at the library boundary: every _lib.call of a step by entry point, and for each call of the deterministic step the
kernels it launches beyond what the same call launches by default (ADDED below: the rules of the launchers in csrc/, evaluated on the
call's own arguments - kernel family of the descriptor, whether default mode already takes the slab form, whether db is passed).
No device: the tool fails (it does not fall back)."""
import argparse
import collections
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--model", choices=("sfd", "dan_deform"), default="sfd")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deterministic: no GPU")
    from dan_amd import _lib, ops, synthetic
    from dan_amd.train_sfd import AnchorConfig, SFDModel, SFDTrainer
    dev = torch.device("cuda:0")
    B, S = a.batch, a.size
    imgs = synthetic.make_images(B, S, S, dev, seed=17)
    if a.model == "sfd":
        loc_t, cls_t, _ = AnchorConfig(S, S, dev).encode_batch(synthetic.make_gt_boxes(B, S, S, seed=5, max_faces=6))
        targets = (loc_t, cls_t)
        trainers = {"default": SFDTrainer(SFDModel(device=dev, seed=11)), "deterministic": SFDTrainer(SFDModel(device=dev, seed=11), deterministic=True)}
    else:
        from dan_amd.train_dan import DANModel, DANTrainer, dan_anchor_config, encode_batch_dan
        anchors = dan_anchor_config(S, S, dev)
        targets = encode_batch_dan(anchors, synthetic.make_gt_boxes(B, S, S, seed=5, max_faces=6))
        trainers = {"default": DANTrainer(DANModel(device=dev, seed=11, deform=True), anchors),
                    "deterministic": DANTrainer(DANModel(device=dev, seed=11, deform=True), anchors, ops_ctx=ops.deterministic_context())}
    for tr in trainers.values():
        for _ in range(a.warmup):
            tr.train_step(imgs, *targets)
    torch.cuda.synchronize()
    # ---- entry-point calls of one step, by name; for the deterministic step also what each call adds in kernel launches
    L = _lib.lib()
    wgrad_calls = []                                          # (descriptor copy, db passed) of every weight-gradient call
    simple = collections.Counter()

    def note(fn, args):
        if fn in ("danhip_conv2d_bwd_weight_ws", "danhip_conv2d_bwd_weight_strided"):
            wgrad_calls.append((_lib.ConvDesc.from_buffer_copy(args[0]._obj), args[4] is not None))
        elif fn in ("danhip_l2norm_bwd_ws", "danhip_l2norm_bwd_pool_scatter_ws", "danhip_detection_loss_fwd_ws"):
            simple[fn] += 1                                   # one ordered reduction
        elif fn == "danhip_relu_bwd_bias_grad_ws" and args[2] is not None:
            simple[fn] += 1
        elif fn == "danhip_deform_conv_bwd_deliver":
            simple[fn + " (far corners: count, 3 x scan, fill, sum instead of the lazy zero and the two empty scatter-form launches)"] += 3
        elif fn == "danhip_sgd_momentum_flat_ws":
            simple[fn] += 2                                   # [rows][64] -> 64 -> 1

    calls = {}
    real_call = _lib.call
    for name, tr in trainers.items():
        cnt = collections.Counter()

        def counting(fn, *args, _cnt=cnt, _det=(name == "deterministic")):
            _cnt[fn] += 1
            if _det:
                note(fn, args)
            return real_call(fn, *args)

        _lib.call = ops.call = counting
        import dan_amd.trainer as trainer_mod
        trainer_mod.call = counting
        try:
            tr.train_step(imgs, *targets)
        finally:
            _lib.call = ops.call = trainer_mod.call = real_call
        torch.cuda.synchronize()
        calls[name] = cnt
    import ctypes
    added = collections.Counter(simple)
    for d, has_db in wgrad_calls:                             # (evaluated with the option at 0: what default mode does for the same call)
        label = L.danhip_conv_wgrad_kernel_label(ctypes.byref(d)).decode()
        slab_family = label.startswith("conv_wgrad_rows_kernel") or label == "conv_wgrad_pw_kernel"
        if slab_family:                                       # combine pass unless default mode takes it too, + db's ordered reduction
            n = (0 if L.danhip_conv2d_bwd_weight_workspace_bytes(ctypes.byref(d)) > 0 else 1) + int(has_db)
        else:                                                 # generic tiles / first layer: ordered reductions of dW and of db
            n = 1 + int(has_db)
        added["weight gradient, " + label.split("<")[0]] += n
    launching = lambda c: sum(v for k, v in c.items() if k != "danhip_set_option")
    added["kernels of calls default mode does not make (conv1_1's weight gradient on its own)"] = launching(calls["deterministic"]) - launching(calls["default"])
    # ---- timing, alternating
    times = {k: [] for k in trainers}
    for _ in range(a.rounds):
        for name, tr in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                tr.train_step(imgs, *targets)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.steps)
    lines = ["# Deterministic mode: cost of the %s step (%d x %d, batch %d, %s)" % ({"sfd": "S3FD", "dan_deform": "DAN-Deform"}[a.model], S, S, B, _lib.ACT_NAME), "",
             "`python tools/bench_deterministic.py --model %s --batch %d --size %d --steps %d --rounds %d`, one process, alternating windows of %d eager steps." % (
                 a.model, B, S, a.steps, a.rounds, a.steps), "", "| mode | ms / step per round | median | img/s |", "|---|---|---|---|"]
    med = {}
    for name, ts in times.items():
        med[name] = sorted(ts)[len(ts) // 2]
        lines.append("| %s | %s | %.3f | %.1f |" % (name, ", ".join("%.3f" % t for t in ts), med[name], B * 1000.0 / med[name]))
    lines += ["", "deterministic / default = %.4f" % (med["deterministic"] / med["default"]), "", "## Entry-point calls per step that differ", "",
              "| entry point | default | deterministic |", "|---|---|---|"]
    for fn in sorted(set(calls["default"]) | set(calls["deterministic"])):
        c0, c1 = calls["default"][fn], calls["deterministic"][fn]
        if c0 != c1:
            lines.append("| `%s` | %d | %d |" % (fn, c0, c1))
    n0, n1 = sum(calls["default"].values()), sum(calls["deterministic"].values())
    lines += ["", "Library calls per step: %d default, %d deterministic." % (n0, n1), "", "## Kernel launches the mode adds per step: %d" % sum(added.values()), "",
              "| where | added launches |", "|---|---|"]
    for k in sorted(added):
        lines.append("| %s | %d |" % (k, added[k]))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
