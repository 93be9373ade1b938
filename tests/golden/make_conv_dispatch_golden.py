"""Records tests/golden/conv_dispatch.json: which kernel instance the convolution dispatch picks, and what its capability and
workspace queries answer, over a grid of descriptors.

    python tests/golden/make_conv_dispatch_golden.py PARENT_LIBDIR [--out tests/golden/conv_dispatch.json]

RUN THIS AGAINST THE PARENT COMMIT'S BUILD: the table is the behaviour a change of the dispatch code has to reproduce
(tests/test_conv_dispatch_cpu.py compares the current build against it), so it is recorded from libdanhip.so / libdanhip_f16.so of
the commit BEFORE that change, never from the build under test.  The label and query functions are host code: no GPU is needed (the
CU count falls back to 256, the MI355X's own).  No DANHIP_* variable may be set: the table is that of the default options.

Two kinds of entry are not the parent's own answer (launch_corrections below; "corrected" in the file counts them): the parent's label
function was a hand-written mirror of its launch path, and there it named another kernel than that launch path ran.  These entries
hold the label of the kernel the parent launched, which is also read from the parent's build, as its label of the call the launch
path really made.

Layout of the file: "names" is the list of kernel-instance labels; per build ("bf16", "fp16") every recorded column is run-length
encoded as [value, count, value, count, ...] over descriptors() in order; label columns hold indices into "names".
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))      # run as a script: the repository root
from dan_amd._lib import ConvDesc, bind as bind_prototypes

NS = (1, 2, 16)
MAPS = ((5, 5), (8, 8), (10, 10), (16, 16), (20, 20), (24, 32), (32, 32), (40, 40), (48, 48), (32, 64), (64, 64), (160, 160))
VALID_MAPS = ((10, 10), (24, 32), (32, 32))       # 3x3 'valid' output sizes (strides 1 and 2) on top of the 'same' grid
CINS = (8, 64, 72, 128, 512, 1024)
COUTS = (4, 8, 16, 24, 40, 64, 72, 128, 256, 512)
KERNELS = (1, 3)
STRIDES = (1, 2, 3)
WHICH = (0, 1, 4, 5, 16, 17, 20, 21)              # danhip_conv_kernel_label codes: forward, data gradient, forward + pool, masked data gradient; | 16 = no scratch

LABEL_COLUMNS = ["label_%d" % w for w in WHICH] + ["wgrad_label"]
VALUE_COLUMNS = ["ws_fwd_q", "ws_fwd_r", "ws_bwd_q", "ws_bwd_r", "ws_wgrad", "pool_only", "emits_bits", "emits_bits_pool", "takes_bits", "first_supported", "concat2",
                 "packed_rows_f", "packed_cols_f", "packed_rows_b", "packed_cols_b"]


# Families that take a call whether or not it carries a bias: the first-layer kernel (its eligibility never looked at the bias) and the
# halo kernel's thin-head instances (danhip_launch_conv_halo: dgrad = ... && !head).
BIAS_BLIND = ("conv3x3_c8_kernel<true>", "conv3x3_halo_kernel<8, 32, 64, 8, 1, 3, 3, false, 1, false>", "conv3x3_halo_kernel<16, 16, 64, 8, 1, 3, 3, false, 1, false>")


def descriptors():
    """The grid, in the order the columns are recorded: (N, H, W, Cin, Ho, Wo, Cout, k, k, stride)."""
    out = []
    for k in KERNELS:
        for cin in CINS:
            for cout in COUTS:
                for s in STRIDES:
                    for (h, w) in MAPS:
                        for n in NS:
                            out.append((n, h, w, cin, (h + s - 1) // s, (w + s - 1) // s, cout, k, k, s))
                    if k == 3 and s <= 2:
                        for (h, w) in VALID_MAPS:
                            for n in NS:
                                out.append((n, h, w, cin, (h - k) // s + 1, (w - k) // s + 1, cout, k, k, s))
    return out


def bind(L):
    """The functions sweep() calls and nothing else: the parent commit's build need not export everything the present header declares."""
    return bind_prototypes(L, ["danhip_conv_kernel_label", "danhip_conv_wgrad_kernel_label", "danhip_conv2d_workspace_bytes",
                               "danhip_conv2d_bwd_weight_workspace_bytes", "danhip_conv2d_fwd_pool_only", "danhip_conv2d_fwd_emits_bits",
                               "danhip_conv2d_bwd_data_takes_bits", "danhip_conv2d_bwd_data_first_supported",
                               "danhip_conv2d_fwd_concat2_supported", "danhip_conv_packed_dims"])


def sweep(L):
    """{column: list over descriptors()}: labels as strings, everything else as integers."""
    cols = {c: [] for c in LABEL_COLUMNS + VALUE_COLUMNS}
    rows, cc = ctypes.c_int64(0), ctypes.c_int64(0)
    for t in descriptors():
        d = ConvDesc(*t)
        p = ctypes.byref(d)
        for w in WHICH:
            cols["label_%d" % w].append(L.danhip_conv_kernel_label(p, w).decode())
        cols["wgrad_label"].append(L.danhip_conv_wgrad_kernel_label(p).decode())
        # the split-K scratch is a whole number of fp32 output maps: recorded exactly as quotient and remainder by one map's bytes, which
        # run-length encodes (the raw byte counts differ from descriptor to descriptor)
        for name, which, unit in (("ws_fwd", 0, 4 * d.N * d.Ho * d.Wo * d.Cout), ("ws_bwd", 1, 4 * d.N * d.H * d.W * d.Cin)):
            q, r = divmod(L.danhip_conv2d_workspace_bytes(p, which), unit)
            cols[name + "_q"].append(q)
            cols[name + "_r"].append(r)
        cols["ws_wgrad"].append(L.danhip_conv2d_bwd_weight_workspace_bytes(p))
        cols["pool_only"].append(L.danhip_conv2d_fwd_pool_only(p))
        cols["emits_bits"].append(L.danhip_conv2d_fwd_emits_bits(p, 0))
        cols["emits_bits_pool"].append(L.danhip_conv2d_fwd_emits_bits(p, 1))
        cols["takes_bits"].append(L.danhip_conv2d_bwd_data_takes_bits(p))
        cols["first_supported"].append(L.danhip_conv2d_bwd_data_first_supported(p))
        cols["concat2"].append(L.danhip_conv2d_fwd_concat2_supported(p, d.Cin // 2, d.Cin))
        for which, (rn, cn) in ((0, ("packed_rows_f", "packed_cols_f")), (1, ("packed_rows_b", "packed_cols_b"))):
            rc = L.danhip_conv_packed_dims(p, which, ctypes.byref(rows), ctypes.byref(cc))
            cols[rn].append(rows.value if rc == 0 else -1)
            cols[cn].append(cc.value if rc == 0 else -1)
    return cols


def launch_corrections(L, cols):
    """Returns the number of entries changed, per kind.

    Data gradient without mask (codes 1 and 17) of a stride-1 descriptor: the parent's launch_conv got the arguments of a forward call of
    the transposed descriptor (Cout rounded up to 8 -> Cin over the output map, pad' = k - 1 - pad) without bias, and tried the families in
    the forward's order.  danhip_conv_kernel_label asked the first-layer kernel on forward codes only and danhip_conv_halo_label said "not
    mine" for a thin head when told dgrad, so both named the flat-M kernel; the launch ran the BIAS_BLIND family.  Which calls these are is
    what the parent's own forward label of the transposed descriptor (codes 0 and 16) says.

    Forward + pool (codes 4 and 20) where the label names the flat-M kernel, which never pools in its epilogue: danhip_conv2d_fwd_pool_arg
    cleared pool_y for such a shape (danhip_conv_pool_fusable was false), launched it as the plain forward call without scratch and ran
    the pool kernel after it.  The label kept pool_y, and the streaming GEMM's eligibility (conv_pointwise.hip: "a.pool_y -> false")
    declined what it then ran.  The call made is the one code 16 describes."""
    n = [0, 0]
    for i, (N, H, W, cin, Ho, Wo, cout, k, _, s) in enumerate(descriptors()):
        if s == 1:
            t = ConvDesc(N, Ho, Wo, (cout + 7) // 8 * 8, H, W, cin, k, k, 1)
            for col, fwd_code in (("label_1", 0), ("label_17", 16)):
                ran = L.danhip_conv_kernel_label(ctypes.byref(t), fwd_code).decode()
                if ran in BIAS_BLIND and cols[col][i] != ran:
                    assert cols[col][i].startswith("conv_igemm_kernel<"), (col, i, cols[col][i], ran)
                    cols[col][i] = ran
                    n[0] += 1
        for col in ("label_4", "label_20"):
            if cols[col][i].startswith("conv_igemm_kernel<") and cols[col][i] != cols["label_16"][i]:
                cols[col][i] = cols["label_16"][i]
                n[1] += 1
    return n


def rle(values):
    out = []
    for v in values:
        if out and out[-2] == v:
            out[-1] += 1
        else:
            out += [v, 1]
    return out


def unrle(pairs):
    out = []
    for i in range(0, len(pairs), 2):
        out += [pairs[i]] * pairs[i + 1]
    return out


def load(path):
    """The recorded table as {"bf16" / "fp16": {column: list over descriptors()}} with labels as strings again."""
    with open(path) as f:
        g = json.load(f)
    names = g["names"]
    out = {}
    for build in ("bf16", "fp16"):
        cols = {c: unrle(v) for c, v in g[build].items()}
        for c in LABEL_COLUMNS:
            cols[c] = [names[i] for i in cols[c]]
        out[build] = cols
    assert g["descriptors"] == len(descriptors()), "the grid of descriptors() is not the one the table was recorded over"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libdir", help="directory holding libdanhip.so and libdanhip_f16.so of the PARENT commit")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_dispatch.json"))
    args = ap.parse_args()
    assert not [k for k in os.environ if k.startswith("DANHIP_")], "unset every DANHIP_* variable: the table is that of the default options"
    builds = (("bf16", "libdanhip.so"), ("fp16", "libdanhip_f16.so"))
    tables, corrected = {}, {}
    for b, so in builds:
        L = bind(ctypes.CDLL(os.path.join(os.path.abspath(args.libdir), so)))
        tables[b] = sweep(L)
        corrected[b] = launch_corrections(L, tables[b])
    names = sorted({v for t in tables.values() for c in LABEL_COLUMNS for v in t[c]})
    index = {n: i for i, n in enumerate(names)}
    g = {"descriptors": len(descriptors()), "names": names, "corrected": corrected}
    for b, t in tables.items():
        g[b] = {c: rle([index[v] for v in t[c]] if c in LABEL_COLUMNS else t[c]) for c in LABEL_COLUMNS + VALUE_COLUMNS}
    with open(args.out, "w") as f:
        json.dump(g, f, separators=(",", ":"))
        f.write("\n")
    print("%d descriptors, %d labels, launch corrections %r -> %s (%d bytes)" % (len(descriptors()), len(names), corrected, args.out, os.path.getsize(args.out)))
    for n in names:
        print("  ", n)


if __name__ == "__main__":
    main()
