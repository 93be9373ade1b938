"""danhip_deform_sample_bwd alone at 160 x 160 x 256, batch 16 (bf16 build): default mode against deterministic mode (the ordered far-corner
path, csrc/deform_far.hip), alternating in one process, for offsets N(0, 0.5 px) and N(0, 2 px).

    python tools/bench_deform_bwd_ordered.py [--rounds 5] [--calls 5]

Per round and mode: `calls` calls between two device events, one synchronise at the end.  Prints the rounds, the median, the spread and
the workspace of each mode.  No device: the tool fails."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deform_bwd_ordered: no GPU")
    from dan_amd import _lib, ops
    from dan_amd._lib import call, ptr, stream
    dev = torch.device("cuda:0")
    N, H, W, C, dg = 16, 160, 160, 256, 4
    g = torch.Generator().manual_seed(0)
    x = torch.randn((N, H, W, C), generator=g).to(ops.ACT).to(dev)
    dS = torch.randn((N * H * W, 9 * C), generator=g).to(ops.ACT).to(dev)
    dx, nws = torch.empty_like(x), {"default": (N * H * W * C + 64) * 4,
                                    "ordered": int(_lib.lib().danhip_deform_sample_bwd_ordered_workspace_bytes(N, H, W, C, dg))}
    ws = torch.empty(nws["ordered"] // 4, dtype=torch.float32, device=dev)
    print("workspace: default %.1f MB, ordered %.1f MB (+%.1f MB)" % (nws["default"] / 1e6, nws["ordered"] / 1e6, (nws["ordered"] - nws["default"]) / 1e6))
    for sigma in (0.5, 2.0):
        off = (torch.randn((N, H, W, dg * 18), generator=g) * sigma).to(ops.ACT).to(dev)
        doff = torch.empty_like(off)
        far1 = int(((off.float().view(-1, 2) < -1) | (off.float().view(-1, 2) >= 1)).any(dim=1).sum().item())
        far2 = int(((off.float().view(-1, 2) < -2) | (off.float().view(-1, 2) >= 2)).any(dim=1).sum().item())

        def run(mode):
            call("danhip_deform_sample_bwd", ptr(x), ptr(off), ptr(dS), ptr(dx), ptr(doff), N, H, W, C, 3, 3, 1, 1, dg, 0, ptr(ws), nws[mode], stream())

        times = {"default": [], "ordered": []}
        for r in range(a.rounds + 1):                                      # (round 0 warms up)
            for mode in ("default", "ordered"):
                call("danhip_set_option", b"deterministic", 1 if mode == "ordered" else 0)
                try:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.calls):
                        run(mode)
                    e1.record()
                    torch.cuda.synchronize()
                finally:
                    call("danhip_set_option", b"deterministic", 0)
                if r:
                    times[mode].append(e0.elapsed_time(e1) / a.calls)
        pairs = off.numel() // 2
        print("offsets N(0, %.1f px): %.1f %% of the taps outside [-1, 1), %.1f %% outside [-2, 2)" % (sigma, 100.0 * far1 / pairs, 100.0 * far2 / pairs))
        for mode, ts in times.items():
            ts = sorted(ts)
            print("  %-8s ms per call: %s  median %.3f  spread %.3f" % (mode, ", ".join("%.3f" % t for t in ts), ts[len(ts) // 2], ts[-1] - ts[0]))


if __name__ == "__main__":
    main()
